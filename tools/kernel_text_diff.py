#!/usr/bin/env python3
"""Per-kernel text diff of two device assembly files (hipcc --cuda-device-only -S of the same source at two
commits).  A function body is the text from its label to its .Lfunc_end label, comments and blank lines
stripped; the bodies are compared as text, symbol by symbol, and nothing else is looked at.

    kernel_text_diff.py OLD.s NEW.s [--show REGEX] [--normalize] [--rename REGEX=REPL ...]

--normalize makes the comparison independent of where a function stands in the file and of its own symbol: the
function index in local labels (.LBB12_3 -> .LBB_3, likewise .LJTI / .Ltmp) and the function's own mangled name are
replaced by placeholders.  It is needed whenever functions are added or removed, which renumbers every later one.
--rename rewrites the demangled names of OLD before pairing (re.sub), for a kernel whose template parameters
changed spelling but not meaning, e.g. --rename 'k_adj_tb<(\d), false>=k_adj_tb<\1, 0>'.

prints `identical N, differing M, only in one file K`, the differing symbols, and with --show the unified diff
of the differing symbols whose (demangled) name matches.  Exit status 1 if anything differs."""
import argparse
import difflib
import re
import subprocess
import sys


def bodies(path, normalize=False):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";", 1)[0].rstrip()
        if normalize and name is not None:
            line = re.sub(r"\.(LBB|LJTI|Ltmp)\d+_", r".\1_", line.replace(name, "@self"))
        if not line.strip():
            continue
        if name is None:
            m = re.match(r"\s*\.type\s+(\S+),@function", line)
            if m:
                name, body = m.group(1), []
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            out[name] = body
            name = None
            continue
        body.append(line)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", default=None, help="print the diff of differing symbols matching this regex")
    ap.add_argument("--normalize", action="store_true", help="ignore function numbering in local labels and own name")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="rewrite OLD's demangled names before pairing (implies pairing by demangled name)")
    args = ap.parse_args()
    a, b = bodies(args.old, args.normalize), bodies(args.new, args.normalize)
    pretty = demangle(sorted(set(a) | set(b)))
    if args.rename:      # pair by demangled name, OLD's rewritten
        def renamed(n):
            for r in args.rename:
                pat, repl = r.split("=", 1)
                n = re.sub(pat, repl, n)
            return n
        a = {renamed(pretty[n]): v for n, v in a.items()}
        b = {pretty[n]: v for n, v in b.items()}
        pretty = {n: n for n in set(a) | set(b)}
    same = [n for n in a if n in b and a[n] == b[n]]
    diff = [n for n in a if n in b and a[n] != b[n]]
    only = sorted(set(a) ^ set(b))
    print(f"functions: {len(a)} old, {len(b)} new; identical {len(same)}, differing {len(diff)}, "
          f"only in one file {len(only)}")
    for n in diff:
        print(f"  differs: {pretty[n]}  ({len(a[n])} -> {len(b[n])} lines)")
    for n in only:
        print(f"  only in {'old' if n in a else 'new'}: {pretty[n]}")
    if args.show:
        for n in diff:
            if re.search(args.show, pretty[n]):
                print(f"\n==== {pretty[n]}")
                sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a[n], b[n], "old", "new", lineterm="", n=2))
    return 1 if diff or only else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Per-kernel text diff of two device assembly files (hipcc --cuda-device-only -S of the same source at two
commits).  A function body is the text from its label to its .Lfunc_end label, comments and blank lines
stripped; the bodies are compared as text, symbol by symbol, and nothing else is looked at.

    kernel_text_diff.py OLD.s NEW.s [--show REGEX]

prints `identical N, differing M, only in one file K`, the differing symbols, and with --show the unified diff
of the differing symbols whose (demangled) name matches.  Exit status 1 if anything differs."""
import argparse
import difflib
import re
import subprocess
import sys


def bodies(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";", 1)[0].rstrip()
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
    args = ap.parse_args()
    a, b = bodies(args.old), bodies(args.new)
    pretty = demangle(sorted(set(a) | set(b)))
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

#!/usr/bin/env python3
"""Instruction histogram (and optionally the text) of one kernel in a `hipcc -S --cuda-device-only` listing:
   tools/isa_kernel.py listing.s <mangled-name prefix> [--dump] [--grep PATTERN]
Comparison of two listings, kernel by kernel (exit status 1 on any difference):
   tools/isa_kernel.py --compare before.s after.s"""
import collections, re, subprocess, sys


def is_ins(l):
    return l.strip() and l.startswith('\t') and not l.startswith('\t.') and not l.startswith('\t;')


def kernels(path):
    """{kernel symbol: its lines from the label to s_endpgm}; lines naming the translation unit's __hip_cuid_ symbol are dropped, and local
    labels and block names lose the function's ordinal in the translation unit (.LBB21_4 -> .LBB_4): it follows the order of instantiation, which host code sets;
    the blanks in front of a trailing comment, which pad to a column after the label's width, shrink to one"""
    s = "\n".join(l for l in open(path).read().splitlines() if '__hip_cuid_' not in l)
    s = re.sub(r'[ \t]+;', ' ;', re.sub(r'(\.L[A-Za-z]+|\bBB)\d+_(\d+)', r'\1_\2', s))      # (block names in the trailing comments too)
    out = {}
    for name in re.findall(r'^\t\.amdhsa_kernel (\S+)', s, re.M):
        start = re.search(r'^' + re.escape(name) + r':', s, re.M).start()
        out[name] = s[start:s.index('.Lfunc_end', start)].splitlines()      # (a kernel with an early return holds several s_endpgm)
    return out


def compare(a, b):
    ka, kb = kernels(a), kernels(b)
    names = sorted(set(ka) | set(kb))
    plain = subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.split('\n')
    differing = 0
    for sym, name in zip(names, plain):
        if sym not in ka or sym not in kb: verdict = "only in " + (a if sym in ka else b)
        elif ka[sym] == kb[sym]: verdict = "identical"
        else: verdict = f"differs (instructions {sum(map(bool, map(is_ins, ka[sym])))} -> {sum(map(bool, map(is_ins, kb[sym])))})"
        differing += verdict != "identical"
        print(f"{verdict:12s} {name}")
    print(f"{len(ka)} kernels in {a}, {len(kb)} in {b}: {differing} differing or unmatched")
    return 1 if differing else 0


if sys.argv[1] == "--compare":
    sys.exit(compare(sys.argv[2], sys.argv[3]))
name = sys.argv[2]
lines = next(v for k, v in kernels(sys.argv[1]).items() if k.startswith(name))      # the whole function, every s_endpgm of it
ins = [l for l in lines if is_ins(l)]
print("instructions:", len(ins))
cnt = collections.Counter(l.split()[0] for l in ins)
print(" ".join(f"{k}:{v}" for k, v in cnt.most_common(60)))
if "--dump" in sys.argv:
    print("\n".join(lines))
if "--grep" in sys.argv:
    pat = sys.argv[sys.argv.index("--grep") + 1]
    for i, l in enumerate(lines):
        if re.search(pat, l): print(i, l)

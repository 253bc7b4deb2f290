#!/usr/bin/env python3
"""Vector and scalar instructions of the common step of the v4 primary march loop -- the ray stays inside its anchor and
needs no further descent -- in the assembly of one kernel.

    hipcc --offload-arch=gfx950 -O3 ... --cuda-device-only -S -o k.s vrt_launch_primary.hip
    python3 tools/march_step_count.py k.s [kernel-name-substring] [--list]

The path is followed from the loop header (the last depth-1 loop header of the kernel): the header up to its first branch
(the "left the anchor" block is skipped), the join and the "status is kGo" test, the cell load and the "subdivided" test,
then the planes block and the latch up to the back edge. tools/isa_cost.py --blocks prices the same blocks."""
import re, sys
args = [a for a in sys.argv[1:] if not a.startswith('--')]
name = args[1] if len(args) > 1 else 'ILi0ENS_2v45TravTILb1EEELi64ELi7ELi1EEE'
src = open(args[0]).read().split('\n')
start = next(i for i, l in enumerate(src) if l.startswith('_Z') and name in l.split(':')[0] and ':' in l)
end = next(i for i in range(start, len(src)) if 's_endpgm' in src[i])
lines = src[start:end + 1]
def label_idx(lab):
    for i, l in enumerate(lines):
        if l.startswith(lab + ':'): return i
    raise KeyError(lab)
# header: the loop header whose body holds the in-anchor test
hdr = [i for i, l in enumerate(lines) if 'This Loop Header: Depth=1' in l]
segs = []
h = hdr[-1]
i = h
# segment 1: from header to first s_cbranch_execz (skip to the in-anchor join)
def take_until_branch(i):
    seg = []
    while True:
        seg.append(lines[i])
        if lines[i].strip().startswith('s_cbranch'): return seg, lines[i].split()[-1]
        i += 1
s1, j1 = take_until_branch(h)
i = label_idx(j1)                  # join after !in_anchor block
s2, _ = take_until_branch(i)       # status == kGo test
i += len(s2)                       # fall through: load block
while not lines[i].strip() or lines[i].strip().startswith(';'): i += 1
s3, j3 = take_until_branch(i)      # load + "subdivided" test -> jumps to planes block
i = label_idx(j3)
s4 = []
while True:                        # planes block + latch up to the back edge
    s4.append(lines[i])
    if lines[i].strip().startswith('s_cbranch_execz') and len(s4) > 3: break
    i += 1
body = [l.strip() for l in s1 + s2 + s3 + s4 if l.strip() and not l.strip().startswith(';') and not l.strip().startswith('.')]
v = [l for l in body if l.startswith('v_') or l.startswith('global_')]
s = [l for l in body if l.startswith('s_')]
print(f"common step: {len(v)} vector (incl. {sum(1 for l in v if l.startswith('global_'))} load), {len(s)} scalar "
      f"({sum(1 for l in s if l.startswith('s_nop'))} s_nop, {sum(1 for l in s if l.startswith('s_waitcnt'))} s_waitcnt, {sum(1 for l in s if l.startswith('s_cbranch'))} branch)")
if '--list' in sys.argv:
    print('\n'.join(body))

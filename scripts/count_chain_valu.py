#!/usr/bin/env python3
"""Instruction counts of the chained body kernels' hot blocks (conv_chain.s, made by `make check`).

For every basic block with at least 100 v_mfma instructions: the number of v_mfma and of other v_* instructions
(v_accvgpr_* moves excluded), and per kernel its .sgpr_spill_count.  Instructions are classified by these prefixes
only.  Every VALU instruction between two MFMAs of a wave adds to the MFMA time, so the count of a hot
block is what the fixed-geometry instances (Geo41) are built to keep down: the run fails when one of
them exceeds the ceilings below.

A 5-row tile of 41 pixels is 13 sub-tiles: one group of 4 and three of 3.  The generic instance runs them through a loop
over two hot blocks (one per group size) plus 21 v_mov of register copies on the loop's back edge per group; the fixed
instance issues a full tile as ONE straight-line block and keeps the two loop blocks for the 1-row tile that ends an image.

    other v_* per block              generic instance            fixed instance (= ceiling)
    forward / unmasked dgrad
      full tile (1872 MFMA)          37 + 3 x 49 = 184 (+ 84)    83
      4 sub-tiles (576 MFMA)         37                          23
      3 sub-tiles (432 MFMA)         49                          33
    masked dgrad
      full tile                      57 + 3 x 63 = 246 (+ 84)    157
      4 sub-tiles                    57                          39
      3 sub-tiles                    63                          49
    .sgpr_spill_count                16 / 57 (masked)            4 / 47 (masked)

What remains in a forward tile: 56 v_max_i32 (the ReLU of 14 parked sub-tiles: the group the tile inherits runs all four
slots, its size being unknown at compile time, then 4 + 3 + 3), 24 v_add_u32 (the LDS addresses of the staging commits) and 3
v_add_u32 of the table cursor.  The masked data gradient has a v_cmp + v_cndmask pair where the forward pass has a v_max,
plus 17 v_readlane of scalar spills per tile and one v_mov: with the mask's buffer resource and the six staging masks its
scalar registers do not fit.  The two loop blocks of the fixed instances run once per image (its last, 1-row tile); their 3
sub-tile block still copies the parked registers before the epilogue (8 v_mov_b64), which the compiler could not be talked
out of from C++.
"""
import re
import sys

HOT = 100
# kernel-name fragment of a fixed instance -> ({v_mfma of a hot block: ceiling of its other v_*}, sgpr spill ceiling)
CEIL = {
    'conv_chain_kernelILb0ELi0ENS_5Geo41E': ({1872: 83, 576: 23, 432: 33}, 4),
    'conv_chain_kernelILb1ELi1ENS_5Geo41E': ({1872: 157, 576: 39, 432: 49}, 47),
    'conv_chain_kernelILb1ELi0ENS_5Geo41E': ({1872: 83, 576: 23, 432: 33}, 4),
}


def blocks(path):
    """-> [(kernel, label, n_mfma, n_valu)], {kernel: sgpr spills}"""
    out, spills = [], {}
    kernel, label, nm, nv = None, None, 0, 0
    name = None
    for l in open(path):
        t = l.strip()
        m = re.match(r'([A-Za-z_.$][\w.$]*):', t)
        if m and not l.startswith(('\t', ' ')):
            if kernel is not None:
                out.append((kernel, label, nm, nv))
            if not m.group(1).startswith('.L'):
                kernel = m.group(1)
            label, nm, nv = m.group(1), 0, 0
            continue
        if t.startswith('.name:'):
            name = t.split()[1]
        elif t.startswith('.sgpr_spill_count:') and name:
            spills[name] = int(t.split()[1])
        if not l.startswith('\t') or kernel is None:
            continue
        op = t.split()[0] if t else ''
        if op.startswith('v_mfma'):
            nm += 1
        elif op.startswith('v_') and not op.startswith('v_accvgpr_'):
            nv += 1
    if kernel is not None:
        out.append((kernel, label, nm, nv))
    return out, spills


def main(paths):
    bad = 0
    for path in paths:
        blks, spills = blocks(path)
        for kernel, label, nm, nv in blks:
            if nm < HOT:
                continue
            ceil = [c for k, c in CEIL.items() if k in kernel]
            note = ''
            if ceil and nv > ceil[0][0].get(nm, -1):
                note = '   <-- above the ceiling of %d' % ceil[0][0].get(nm, -1)
                bad += 1
            print('%-72s %-10s %4d v_mfma %4d other v_*%s' % (kernel, label, nm, nv, note))
        for name, n in sorted(spills.items()):
            ceil = [c for k, c in CEIL.items() if k in name]
            note = ''
            if ceil and n > ceil[0][1]:
                note = '   <-- above the ceiling of %d' % ceil[0][1]
                bad += 1
            print('%-72s .sgpr_spill_count %d%s' % (name, n, note))
    print('%d counts above their ceilings' % bad)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))

#!/usr/bin/env python3
"""Instruction counts of the hot blocks of the chained body kernels (conv_chain.s) and of the exact-row filter gradient
(wgrad_batch.s, wgrad_pipe_inst.s), all made by `make check`.

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
    .sgpr_spill_count                16 / 57 (masked)            2 (forward) / 4 / 47 (masked)

The full tile's staging writes go to constant LDS slots (two per-lane bases per tile + immediates, FixedSlots): before that
a full tile had 24 v_add_u32 of LDS addresses more -- 83 other v_* (forward, unmasked data gradient) and 157 (masked), now 61
and 135.

What remains in a forward tile: 56 v_max_i32 (the ReLU of 14 parked sub-tiles: the group the tile inherits runs all four
slots, its size being unknown at compile time, then 4 + 3 + 3), 2 v_add_u32 of the staging bases and 3 v_add_u32 of the table
cursor.  The masked data gradient has a v_cmp + v_cndmask pair where the forward pass has a v_max,
plus 17 v_readlane of scalar spills per tile and one v_mov: with the mask's buffer resource and the six staging masks its
scalar registers do not fit.  The two loop blocks of the fixed instances run once per image (its last, 1-row tile); their 3
sub-tile block still copies the parked registers before the epilogue (8 v_mov_b64), which the compiler could not be talked
out of from C++.

Exact-row filter gradient (wgrad_rows_full_kernel, wgrad_rows_batch_kernel: one body).  A 3-row unit is one block of 1116
MFMAs; the other blocks of the unit loop run once per unit (the drain loop nested in it: never in a full window, not
counted).  Counts of other v_*, the same in both kernels, before and after the staging writes took constant slots and the
bias-gradient sum moved in front of the window handover:

                                     before                              now (= ceiling)
    the 1116-MFMA block              39 (15 of them LDS address adds)    55 = 24 + the 31 v_add_f32 of the bias gradient
    once per unit outside it         69 (31 v_add_f32 + 31 v_mov_b32     8 (1 flip of the staging base, 7 of the tile
                                     of the handover, 7 others)          descriptor)
    per unit                         108                                 63

The 31 additions of the bias gradient cannot leave the unit; they used to sit on the loop's back edge, where they kept the old
window's registers alive across the handover, which therefore read the new window into other registers and copied it home.
"""
import re
import sys

HOT = 100
# kernel-name fragment -> ({v_mfma of a hot block: ceiling of its other v_*}, sgpr spill ceiling,
#                          {v_mfma of a hot block: ceiling of the other v_* in the rest of its loop, inner loops excluded})
CEIL = {
    'conv_chain_kernelILb0ELi0ENS_5Geo41E': ({1872: 61, 576: 23, 432: 33}, 2, {}),
    'conv_chain_kernelILb1ELi1ENS_5Geo41E': ({1872: 135, 576: 39, 432: 49}, 47, {}),
    'conv_chain_kernelILb1ELi0ENS_5Geo41E': ({1872: 61, 576: 23, 432: 33}, 4, {}),
    'wgrad_rows_full_kernelILi3ELi3ELi64ELi4ELi41E': ({1116: 55}, 0, {1116: 8}),
    'wgrad_rows_batch_kernelILi3ELi3ELi64ELi4ELi41E': ({1116: 55}, 0, {1116: 8}),
}
LOOP = re.compile(r';\s+(?:in Loop: Header=(BB\w+)|(=>)\s*This Loop Header:) Depth=(\d+)')


def blocks(path):
    """-> [(kernel, label, n_mfma, n_valu, loop)], {kernel: sgpr spills}; loop = the label of the innermost loop's header when
    the block belongs to that loop directly (the compiler's annotation of the label), else None"""
    out, spills = [], {}
    kernel, label, nm, nv, loop = None, None, 0, 0, None
    name = None
    for l in open(path):
        t = l.strip()
        m = re.match(r'([A-Za-z_.$][\w.$]*):', t)
        if m and not l.startswith(('\t', ' ')):
            if kernel is not None:
                out.append((kernel, label, nm, nv, loop))
            if not m.group(1).startswith('.L'):
                kernel = m.group(1)
            label, nm, nv = m.group(1), 0, 0
            lm = LOOP.search(l)
            loop = None if not lm else (label if lm.group(2) else '.L' + lm.group(1))
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
        out.append((kernel, label, nm, nv, loop))
    return out, spills


def main(paths):
    bad = 0
    for path in paths:
        blks, spills = blocks(path)
        for kernel, label, nm, nv, loop in blks:
            if nm < HOT:
                continue
            ceil = [c for k, c in CEIL.items() if k in kernel]
            note = ''
            if ceil and nv > ceil[0][0].get(nm, -1):
                note = '   <-- above the ceiling of %d' % ceil[0][0].get(nm, -1)
                bad += 1
            print('%-72s %-10s %4d v_mfma %4d other v_*%s' % (kernel, label, nm, nv, note))
            if ceil and nm in ceil[0][2]:
                rest = sum(b[3] for b in blks if b[0] == kernel and b[4] == loop and b[1] != label) if loop else -1
                note = ''
                if rest < 0 or rest > ceil[0][2][nm]:
                    note = '   <-- above the ceiling of %d' % ceil[0][2][nm] if loop else '   <-- the block is in no loop'
                    bad += 1
                print('%-72s %-10s the rest of its loop: %4d other v_*%s' % (kernel, label, rest, note))
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

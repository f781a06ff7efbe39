"""Which of its five kernels srx_gemm runs, pinned on the host: a CPU test on the real library, no device.

srx_gemm_route_of is the decision srx_gemm itself makes (one function, gemm_plan in csrc/enet_ops.hip, serves both); it
looks at its pointers (NULL, alignment) and never reads them, so the operands here are addresses of chosen alignment.

CASES is the one table of GEMM shapes: every row names the route it is there to reach, this test asserts that it reaches
it, and tests/test_gpu_exact_loss_side.py imports the table, asserts the route again with the device's pointers and holds
the result to the float64 oracle.  The shapes are the smallest at which each kernel can still go wrong, read off the
predicates of gemm_plan; the boundary rows stand one step outside each predicate, so that a changed constant moves a row."""
import collections
import ctypes

import pytest

Case = collections.namedtuple('Case', 'M N K batch trans_a trans_b bias act ws b_offset route why')

ROUTES = ('tile', 'tile_splitk', 'tile_per_wave', 'skinny_nn', 'skinny_nt')      # ops.GEMM_ROUTES


def case(M, N, K, route, batch=None, ta=False, tb=False, bias=False, act=None, ws=True, b_offset=0, why=''):
    """batch None: 2-D operands.  bias / act: the call carries a bias / this activation.  ws: the caller passes the workspace
    srx_gemm_workspace_bytes asks for (where it asks for none there is none to pass).  b_offset: bytes B lies past a 16-byte
    boundary."""
    return Case(M, N, K, batch, ta, tb, bias, act, ws, b_offset, route, why)


def _forms(M, N, K, route, **kw):
    return [case(M, N, K, route, **kw), case(M, N, K, route, ta=True, **kw), case(M, N, K, route, tb=True, **kw)]


CASES = (
    # ---- TILE: gemm_mfma_kernel, one 64 x 64 tile per workgroup
    _forms(5, 7, 3, 'tile', why='K below one MFMA step') +
    _forms(130, 70, 33, 'tile', why='M and N tails across a 64 tile, K tail') +
    _forms(65, 17, 18, 'tile', batch=3, why='batched') +
    # ---- TILE_SPLITK: K ranges into the workspace + gemm_splitk_finish_kernel
    [case(17, 9, 520, 'tile_splitk', why='8 ranges of 80: the last one empty, K no multiple of 16'),
     case(17, 9, 520, 'tile_splitk', tb=True, why='8 ranges of 80, B transposed'),
     case(64, 64, 1024, 'tile_splitk', why='16 full ranges of 64'),
     case(64, 64, 1024, 'tile_splitk', ta=True, why='16 full ranges of 64, A transposed'),
     case(130, 70, 600, 'tile_splitk', why='6 tiles, 9 ranges of 80: the last one empty'),
     case(130, 70, 600, 'tile_splitk', bias=True, act='relu', why='the epilogue runs in the finish kernel')] +
    # ---- TILE_PER_WAVE: gemm_mfma_w64_kernel, one 64 x 64 tile per wave
    [case(48, 48, 5, 'tile_per_wave', batch=1025, why='1025 units: the last workgroup has one live wave; K < 8'),
     case(100, 49, 9, 'tile_per_wave', batch=600, why='two row tiles with tails'),
     case(4100, 1000, 2, 'tile_per_wave', ta=True, why='1040 tiles of one matrix: a dense layer\'s filter gradient, K = batch'),
     case(48, 48, 5, 'tile_per_wave', batch=1024, bias=True, act='relu', why='exactly 1024 units, with the epilogue')] +
    # ---- SKINNY_NN: gemm_skinny_nn_kernel<4/8/16> + the finish kernel.  K = 4100: 16 ranges of 272, the last holds 20;
    #      N = 260 / 1028: a second column block of one float4
    [case(M, N, K, 'skinny_nn', why='MT %d' % (4 if M <= 4 else 8 if M <= 8 else 16))
     for M in (1, 4, 5, 8, 9, 16) for N in (260, 1028) for K in (4096, 4100)] +
    [case(5, 260, 4100, 'skinny_nn', bias=True, act='relu', why='the epilogue of the skinny forward')] +
    # ---- SKINNY_NT: gemm_skinny_nt_kernel<4/8/16> (B transposed, no bias, no activation)
    [case(3, 2051, 256, 'skinny_nt', tb=True, why='MT 4: four rows of B per trip, N no multiple of 4'),
     case(7, 2049, 512, 'skinny_nt', tb=True, why='MT 8: two rows per trip, one surplus row'),
     case(13, 4100, 768, 'skinny_nt', tb=True, why='MT 16: one row per trip, 4100 trips: the 1024-workgroup grid strides; 48 KiB'),
     case(4, 2048, 3072, 'skinny_nt', tb=True, why='MT 4: exactly 48 KiB of LDS')] +
    # ---- fall-throughs: one step outside a skinny predicate, and where they land
    [case(4, 258, 4096, 'tile_splitk', why='fall-through: NN shape, N = 258 is no multiple of 4'),
     case(4, 260, 4098, 'tile_splitk', why='fall-through: NN shape, K = 4098 is no multiple of 4'),
     case(4, 260, 4096, 'tile_splitk', b_offset=4, why='fall-through: NN shape, B 4 bytes past a 16-byte boundary'),
     case(4, 260, 4096, 'tile', ws=False, why='fall-through: NN shape, no workspace passed'),
     case(4, 2048, 3328, 'tile_splitk', tb=True, why='fall-through: NT shape, 52 KiB of LDS'),
     case(3, 2051, 256, 'tile', tb=True, bias=True, why='fall-through: NT shape with a bias'),
     case(3, 2051, 300, 'tile', tb=True, why='fall-through: NT shape, K = 300 is no multiple of 256')] +
    # ---- boundaries: the nearest shape on the other side of every remaining constant
    [case(48, 48, 5, 'tile', batch=1023, why='boundary: 1023 units'),
     case(47, 48, 5, 'tile', batch=1025, why='boundary: M = 47 is no tile per wave'),
     case(48, 47, 5, 'tile', batch=1025, why='boundary: N = 47 is no tile per wave'),
     case(64, 64, 511, 'tile', why='boundary: K = 511 is not split'),
     case(64, 64, 512, 'tile_splitk', why='boundary: K = 512 is split, 8 ranges of 64'),
     case(512, 1024, 512, 'tile', why='boundary: 128 tiles are not split'),
     case(64, 8128, 512, 'tile_splitk', why='boundary: 127 tiles are split, 3 ranges of 176'),
     case(17, 260, 4096, 'tile_splitk', why='boundary: M = 17 is not skinny'),
     case(4, 252, 4096, 'tile_splitk', why='boundary: N = 252 is below the NN route'),
     case(4, 260, 4092, 'tile_splitk', why='boundary: K = 4092 is below the NN route'),
     case(3, 2047, 256, 'tile', tb=True, why='boundary: N = 2047 is below the NT route'),
     case(17, 2048, 256, 'tile', tb=True, why='boundary: M = 17 is not skinny'),
     case(3, 2051, 256, 'tile', tb=True, act='relu', why='boundary: NT shape with an activation'),
     case(3, 2051, 256, 'tile', tb=True, b_offset=4, why='boundary: NT shape, B 4 bytes past a 16-byte boundary'),
     case(3, 2048, 256, 'tile', batch=2, tb=True, why='boundary: NT shape, two matrices'),
     case(4, 260, 4096, 'tile', batch=2, why='boundary: NN shape, two matrices')])

FALL_THROUGHS = ('N = 258', 'K = 4098', 'B 4 bytes past', 'no workspace passed', '52 KiB of LDS', 'NT shape with a bias', 'K = 300')


def case_id(c):
    return '%s%dx%dx%d%s%s%s%s%s%s-%s' % ('b%d_' % c.batch if c.batch else '', c.M, c.N, c.K, '_ta' if c.trans_a else '', '_tb' if c.trans_b else '',
                                        '_bias' if c.bias else '', '_' + c.act if c.act else '', '' if c.ws else '_nows',
                                        '_boff%d' % c.b_offset if c.b_offset else '', c.route)


def operand_shapes(c):
    """The shapes of A and B as ops.gemm takes them."""
    a = (c.K, c.M) if c.trans_a else (c.M, c.K)
    b = (c.N, c.K) if c.trans_b else (c.K, c.N)
    return ((c.batch,) + a, (c.batch,) + b) if c.batch else (a, b)


# addresses that are never read: A, bias and the workspace on 16-byte boundaries, B where the row puts it
A_ADDR, B_ADDR, BIAS_ADDR, WS_ADDR = 0x10000000, 0x20000000, 0x30000000, 0x40000000


def host_route(c):
    from ml_super_resolution_amd import _lib, ops
    need = _lib.lib().srx_gemm_workspace_bytes(c.M, c.N, c.K, c.batch or 1)
    a_shape, b_shape = operand_shapes(c)
    return ops.gemm_route((a_shape, A_ADDR), (b_shape, B_ADDR + c.b_offset), bias=BIAS_ADDR if c.bias else None, act=c.act,
                          trans_a=c.trans_a, trans_b=c.trans_b, workspace=(WS_ADDR, need) if c.ws and need else None)


@pytest.mark.parametrize('c', CASES, ids=[case_id(c) for c in CASES])
def test_every_row_reaches_the_route_it_names(c):
    route, splits = host_route(c)
    assert route == c.route, '%s: %s' % (case_id(c), c.why)
    assert (splits > 1) == (route in ('tile_splitk', 'skinny_nn'))


def test_the_table_names_every_route_every_skinny_width_and_every_fall_through():
    assert len(set(case_id(c) for c in CASES)) == len(CASES)
    assert set(c.route for c in CASES) == set(ROUTES)
    mt = lambda c: 4 if c.M <= 4 else 8 if c.M <= 8 else 16
    for route in ('skinny_nn', 'skinny_nt'):
        assert set(mt(c) for c in CASES if c.route == route) == {4, 8, 16}, route
    for tag in FALL_THROUGHS:
        rows = [c for c in CASES if c.why.startswith('fall-through') and tag in c.why]
        assert rows and all(c.route in ('tile', 'tile_splitk') for c in rows), tag
    # both epilogue forms of the finish kernel (after the tile kernel and after the skinny forward), and the one of the tile kernels
    for route in ('tile_splitk', 'skinny_nn', 'tile_per_wave'):
        assert any(c.bias and c.act == 'relu' for c in CASES if c.route == route), route


def test_the_split_counts_of_the_rows_that_are_there_for_them():
    """The K ranges the comments of the table count on: an empty last range, a partly filled one, full ones."""
    by = {case_id(c): host_route(c)[1] for c in CASES}
    assert by['17x9x520-tile_splitk'] == 8                   # ranges of 80: 7 x 80 = 560 >= 520
    assert by['64x64x1024-tile_splitk'] == 16
    assert by['130x70x600-tile_splitk'] == 9                 # ranges of 80: 8 x 80 = 640 >= 600
    assert by['64x64x512-tile_splitk'] == 8
    assert by['64x8128x512-tile_splitk'] == 3
    assert by['1x260x4100-skinny_nn'] == 16                  # ranges of 272: 15 x 272 = 4080, the last holds 20
    assert by['16x1028x4096-skinny_nn'] == 16                # ranges of 256
    assert by['4x258x4096-tile_splitk'] == 52                # 5 tiles: ceil(256 / 5)


def test_refusals_and_the_route_enum():
    """Arguments srx_gemm refuses come back as its negative status; the enum values are the ones include/srx.h states."""
    import os
    import re
    from ml_super_resolution_amd import _lib, ops
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, 'include', 'srx.h')).read()
    enum = dict((n.lower(), int(v)) for n, v in re.findall(r'SRX_GEMM_([A-Z_]+) = (\d)', text))
    assert enum == {name: i for i, name in enumerate(ops.GEMM_ROUTES)} and ops.GEMM_ROUTES == ROUTES
    L = _lib.lib()
    d = _lib.GemmDesc(4, 4, 4, 1, 4, 1, 0, 4, 1, 0, 4, 1, 0, 1.0, 0, 0)
    assert L.srx_gemm_route_of(ctypes.byref(d), A_ADDR, B_ADDR, None, None, 0, None) == 0        # (splits is nullable)
    assert L.srx_gemm_route_of(ctypes.byref(d), None, B_ADDR, None, None, 0, None) == -1 and b'null' in L.srx_last_error()
    for field, value, status in (('M', 0, -1), ('K', -3, -1), ('act', 5, -1), ('batch', 65536, -2)):
        bad = _lib.GemmDesc(4, 4, 4, 1, 4, 1, 0, 4, 1, 0, 4, 1, 0, 1.0, 0, 0)
        setattr(bad, field, value)
        assert L.srx_gemm_route_of(ctypes.byref(bad), A_ADDR, B_ADDR, None, None, 0, None) == status, field
    with pytest.raises(_lib.SrxError):
        ops.gemm_route(((4, 4), None), ((4, 4), B_ADDR), workspace=None)
    # a workspace that is too small or off its 16-byte boundary is no workspace
    c = [c for c in CASES if case_id(c) == '64x64x1024-tile_splitk'][0]
    need = L.srx_gemm_workspace_bytes(c.M, c.N, c.K, 1)
    a_shape, b_shape = operand_shapes(c)
    for ws in ((WS_ADDR, need - 4), (WS_ADDR + 4, need)):
        assert ops.gemm_route((a_shape, A_ADDR), (b_shape, B_ADDR), workspace=ws) == ('tile', 1)

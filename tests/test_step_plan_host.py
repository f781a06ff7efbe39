"""The schedule of a ConvStack step, pinned on the host: which launches `forward` + `loss_and_backward` issue, in which
order, through which buffers.  The launching functions of `ops` are replaced by recorders, the host queries stay real
(without a GPU the library plans for 256 compute units, an MI355X's count), so no test here touches a device.

(a) the recorded call sequence of eight stacks -- every literal below was recorded at the commit BEFORE the planners
    existed, from the loops they replace; (b) the planners against the real library; (c) the host queries per step.
A schedule change edits engine.plan_forward / plan_backward and then these sequences."""
import pytest
import torch

from ml_super_resolution_amd import _lib, engine, ops
from ml_super_resolution_amd.engine import ConvStack, LayerSpec
from ml_super_resolution_amd.vdsr import model_vdsr

QUERIES = ('chain_supported', 'bwd_filter_batch_plan', 'bwd_filter_workspace_bytes', 'bwd_filter_batch_workspace_bytes')


def A(i):
    return ('act', i)


def C(k):
    return ('dpre_chain', k)


DY, DLAST = ('dy', 0), ('dpre_last',)


class Recorder(object):
    """Stands in for the launching functions of `ops`: every call becomes one event that names tensors by their key in
    stack._bufs (or 'x' / 'hd') and filters by their layer index.  What is not schedule -- the bias that goes with a
    kernel, padding, activation, precision, weight decay, workspace -- is checked against the layer's spec on the spot."""

    def __init__(self, monkeypatch, stack, x, hd):
        self.stack, self.x, self.hd = stack, x, hd
        self.events, self.queries = [], dict.fromkeys(QUERIES, 0)
        for fn in ('conv2d_fwd', 'conv2d_fwd_chain', 'conv2d_bwd_data', 'conv2d_bwd_data_chain', 'conv2d_bwd_filter',
                   'conv2d_bwd_filter_batch', 'mse_fwd_bwd', 'l2_loss', 'act_bwd', 'rownorm_loss_fwd_bwd'):
            monkeypatch.setattr(ops, fn, getattr(self, fn))
        for fn in QUERIES:
            monkeypatch.setattr(ops, fn, self._counted(fn, getattr(ops, fn)))

    def _counted(self, fn, real):
        def query(*args, **kwargs):
            self.queries[fn] += 1
            return real(*args, **kwargs)
        return query

    def name(self, t):
        if t is None:
            return None
        if t is self.x:
            return 'x'
        if t is self.hd:
            return 'hd'
        for key, buf in self.stack._bufs.items():
            if t is buf:
                return key
        raise AssertionError('a tensor that is neither x, hd nor one of the stack\'s buffers')

    def names(self, ts):
        return [self.name(t) for t in ts]

    def layer(self, t, buf=None, leaf=0):
        """The layer whose kernel (leaf 0) or bias (leaf 1) in the flat buffer `buf` (default: the parameters) t is."""
        st = self.stack
        assert t._base is (st.params if buf is None else buf)
        j = [off for _, off, _, _, _, _ in st.entries].index(t.storage_offset())
        assert j % 2 == leaf and tuple(t.shape) == st.entries[j][3]
        return j // 2

    def _decay(self, i, w_for_decay):
        if self.stack.weight_decay:
            assert self.layer(w_for_decay) == i
        else:
            assert w_for_decay is None

    def conv2d_fwd(self, x, w, bias, padding, act, skip=None, out=None, precision='highest'):
        i = self.layer(w)
        s = self.stack.specs[i]
        assert self.layer(bias, leaf=1) == i and (padding, act, precision) == (s.padding, s.act, self.stack.layer_precision[i])
        self.events.append(('fwd', i, self.name(x), self.name(skip), self.name(out)))
        return out

    def conv2d_fwd_chain(self, xs, ws, biases, outs, padding, act):
        ls = [self.layer(w) for w in ws]
        assert [self.layer(b, leaf=1) for b in biases] == ls
        assert all((padding, act, 'highest') == (self.stack.specs[i].padding, self.stack.specs[i].act, self.stack.layer_precision[i])
                   for i in ls)
        self.events.append(('fwd_chain', ls, self.names(xs), self.names(outs)))
        return outs[-1]

    def conv2d_bwd_data(self, dpre, w, x_shape, padding, x_in=None, in_act=None, out=None, precision='highest'):
        i = self.layer(w)
        assert tuple(x_shape) == tuple(out.shape) and (padding, precision) == (self.stack.specs[i].padding, self.stack.layer_precision[i])
        self.events.append(('dgrad', i, self.name(dpre), self.name(x_in), in_act, self.name(out)))
        return out

    def conv2d_bwd_data_chain(self, dpres, ws, x_ins, outs, x_shape, padding, in_act=None):
        ls = [self.layer(w) for w in ws]
        assert all(tuple(o.shape) == tuple(x_shape) for o in outs)
        assert all(padding == self.stack.specs[i].padding and self.stack.layer_precision[i] == 'highest' for i in ls)
        self.events.append(('dgrad_chain', ls, self.names(dpres), self.names(x_ins), in_act, self.names(outs)))
        return outs[-1]

    def conv2d_bwd_filter(self, x, dpre, w_shape, padding, w_for_decay=None, wd_scale=0.0, dw=None, dbias=None, workspace=None,
                          precision='highest'):
        st = self.stack
        i = self.layer(dw, st.grads)
        assert self.layer(dbias, st.grads, leaf=1) == i and workspace is st._ws and wd_scale == st.weight_decay
        assert (tuple(w_shape), padding, precision) == (st.specs[i].kernel_shape, st.specs[i].padding, st.layer_precision[i])
        self._decay(i, w_for_decay)
        self.events.append(('wgrad', i, self.name(x), self.name(dpre)))

    def conv2d_bwd_filter_batch(self, xs, dpres, dws, dbiases, w_for_decay, wd_scale, padding, workspace=None):
        st = self.stack
        ls = [self.layer(dw, st.grads) for dw in dws]
        assert [self.layer(db, st.grads, leaf=1) for db in dbiases] == ls and workspace is st._ws and wd_scale == st.weight_decay
        assert all(padding == st.specs[i].padding and st.layer_precision[i] == 'highest' for i in ls)
        for k, i in enumerate(ls):
            self._decay(i, None if w_for_decay is None else w_for_decay[k])
        self.events.append(('wgrad_batch', ls, self.names(xs), self.names(dpres)))

    def mse_fwd_bwd(self, pred, target, loss_out, inv_numel=None, accumulate=False, dpred=None):
        assert loss_out is self.stack.loss and inv_numel == 1.0 / pred.numel() and not accumulate
        self.events.append(('mse', self.name(pred), self.name(target), self.name(dpred)))

    def rownorm_loss_fwd_bwd(self, pred, target, row_len, loss_out, dpred=None, norms=None):
        assert loss_out is self.stack.loss and row_len == pred.shape[1] * pred.shape[2]
        self.events.append(('rownorm', self.name(pred), self.name(target), self.name(dpred), self.name(norms)))
        return dpred

    def l2_loss(self, w, scale, loss_out, accumulate=True, mask=None):
        assert w is self.stack.params and scale == self.stack.weight_decay and loss_out is self.stack.loss and accumulate
        self.events.append(('l2',))

    def act_bwd(self, dy, y, act, out=None):
        self.events.append(('act_bwd', self.name(dy), self.name(y), act, self.name(out)))
        return out


def record_step(monkeypatch, specs, x_shape, hook=None, loss_kind='mse', **stack_args):
    """(events, host queries) of forward(x, keep=True) + loss_and_backward(hd) on uninitialised host tensors."""
    stack = ConvStack(specs, device='cpu', **stack_args)
    stack.loss_kind = loss_kind
    x = torch.empty(x_shape)
    hd = torch.empty(stack._shapes(x_shape)[-1])
    rec = Recorder(monkeypatch, stack, x, hd)
    if hook is not None:
        def keep_hook(xx, outs):
            rec.events.append(('hook', rec.name(xx), rec.names(outs)))
            return hook
        stack.forward_keep_hook = keep_hook
    assert stack.forward(x, keep=True) is stack.acts[-1]
    assert rec.names(stack.acts) == ['x'] + [A(i) for i in range(len(specs))] and stack._acts is stack.acts
    assert stack.loss_and_backward(hd) is stack.loss
    return rec.events, rec.queries


@pytest.fixture
def switches():
    """set(chain, batch) for the test; the environment's defaults afterwards."""
    def set_switches(chain, batch):
        ops.set_chain(chain)
        ops.set_wgrad_batch(batch)
    try:
        yield set_switches
    finally:
        ops.set_chain(-1)
        ops.set_wgrad_batch(-1)


def assert_no_more_queries(queries, parent):
    assert all(queries[q] <= n for q, n in zip(QUERIES, parent)), (queries, parent)


# ---- (a) VDSR-5 at the benchmark's shape, the four combinations of the two groupings ----------------------------------
VDSR5_FWD_CHAINED = [('fwd', 0, 'x', None, A(0)),
                     ('fwd_chain', [1, 2, 3], [A(0), A(1), A(2)], [A(1), A(2), A(3)]),
                     ('fwd', 4, A(3), 'x', A(4))]
VDSR5_FWD_PER_LAYER = [('fwd', 0, 'x', None, A(0)), ('fwd', 1, A(0), None, A(1)), ('fwd', 2, A(1), None, A(2)),
                       ('fwd', 3, A(2), None, A(3)), ('fwd', 4, A(3), 'x', A(4))]
VDSR5_LOSS = [('mse', A(4), 'hd', DY), ('l2',)]
VDSR5_BATCH = ('wgrad_batch', [1, 2, 3], [A(0), A(1), A(2)], [C(1), C(2), C(3)])
DX0, DX1, DX2 = ('dx', 0, 64), ('dx', 1, 64), ('dx', 2, 64)
VDSR5 = {
    (1, 1): VDSR5_FWD_CHAINED + VDSR5_LOSS + [
        ('wgrad', 4, A(3), DY),
        ('dgrad', 4, DY, A(3), 'relu', C(3)),
        ('dgrad_chain', [3, 2, 1], [C(3), C(2), C(1)], [A(2), A(1), A(0)], 'relu', [C(2), C(1), C(0)]),
        VDSR5_BATCH,
        ('wgrad', 0, 'x', C(0))],
    (0, 1): VDSR5_FWD_PER_LAYER + VDSR5_LOSS + [
        ('wgrad', 4, A(3), DY),
        ('dgrad', 4, DY, A(3), 'relu', C(3)),
        ('dgrad', 3, C(3), A(2), 'relu', C(2)),
        ('dgrad', 2, C(2), A(1), 'relu', C(1)),
        VDSR5_BATCH,
        ('dgrad', 1, C(1), A(0), 'relu', DX1),
        ('wgrad', 0, 'x', DX1)],
    (1, 0): VDSR5_FWD_CHAINED + VDSR5_LOSS + [
        ('wgrad', 4, A(3), DY),
        ('dgrad', 4, DY, A(3), 'relu', DX1),
        ('dgrad_chain', [3, 2, 1], [DX1, C(2), C(1)], [A(2), A(1), A(0)], 'relu', [C(2), C(1), C(0)]),
        ('wgrad', 3, A(2), DX1),
        ('wgrad', 2, A(1), C(2)),
        ('wgrad', 1, A(0), C(1)),
        ('wgrad', 0, 'x', C(0))],
    (0, 0): VDSR5_FWD_PER_LAYER + VDSR5_LOSS + [
        ('wgrad', 4, A(3), DY),
        ('dgrad', 4, DY, A(3), 'relu', DX1),
        ('wgrad', 3, A(2), DX1),
        ('dgrad', 3, DX1, A(2), 'relu', DX0),
        ('wgrad', 2, A(1), DX0),
        ('dgrad', 2, DX0, A(1), 'relu', DX2),
        ('wgrad', 1, A(0), DX2),
        ('dgrad', 1, DX2, A(0), 'relu', DX1),
        ('wgrad', 0, 'x', DX1)],
}
# (c) the host queries of those steps before the planners existed, in the order of QUERIES: a plan may not ask more
VDSR5_QUERIES = {(1, 1): (7, 1, 5, 1), (0, 1): (7, 1, 5, 1), (1, 0): (7, 1, 5, 0), (0, 0): (7, 1, 5, 0)}


@pytest.mark.parametrize('chain,batch', sorted(VDSR5))
def test_vdsr5_step_sequence(monkeypatch, switches, chain, batch):
    switches(chain, batch)
    events, queries = record_step(monkeypatch, model_vdsr.layer_specs(5), (256, 41, 41, 3), residual=True, weight_decay=1e-4)
    assert events == VDSR5[chain, batch]
    assert_no_more_queries(queries, VDSR5_QUERIES[chain, batch])


# ---- (a) four further stacks ---------------------------------------------------------------------------------------
def SRCNN_SPECS():          # 9-1-5, VALID (srcnn/srcnn.py:100-130)
    return [LayerSpec(9, 3, 64, 'valid', 'relu'), LayerSpec(1, 64, 32, 'valid', 'relu'), LayerSpec(5, 32, 3, 'valid', 'tanh')]


def ESPCN_SPECS():          # r = 3 (espcn/espcn/model_espcn.py:30-62)
    return [LayerSpec(5, 3, 64, 'same', 'tanh'), LayerSpec(3, 64, 32, 'same', 'tanh'), LayerSpec(3, 32, 27, 'same', None)]


def TANH3_SPECS():
    return [LayerSpec(3, 3, 64, 'same', 'tanh'), LayerSpec(3, 64, 64, 'same', 'relu'), LayerSpec(3, 64, 3, 'same', 'tanh')]


def DEEP_SPECS():           # 40 identical body layers between an RGB first and last layer: more than one chain / batch can take
    return ([LayerSpec(3, 3, 64, 'same', 'relu')] + [LayerSpec(3, 64, 64, 'same', 'relu') for _ in range(40)] +
            [LayerSpec(3, 64, 3, 'same', None)])


def As(lo, hi):
    return [A(i) for i in range(lo, hi + 1)]


def Cs(lo, hi):
    return [C(k) for k in range(lo, hi + 1)]


SMALL_BACKWARD = {          # (head gradient, mask activation of layers 2 / 1, channels of layers 1 / 0): the per-layer order
    'srcnn': (DLAST, 'relu', 'relu', 32, 64), 'espcn': (DY, 'tanh', 'tanh', 32, 64), 'tanh3': (DLAST, 'relu', 'tanh', 64, 64)}


def small_backward(kind):
    head, m2, m1, c1, c0 = SMALL_BACKWARD[kind]
    return [('wgrad', 2, A(1), head),
            ('dgrad', 2, head, A(1), m2, ('dx', 2, c1)),
            ('wgrad', 1, A(0), ('dx', 2, c1)),
            ('dgrad', 1, ('dx', 2, c1), A(0), m1, ('dx', 1, c0)),
            ('wgrad', 0, 'x', ('dx', 1, c0))]


FWD3 = [('fwd', 0, 'x', None, A(0)), ('fwd', 1, A(0), None, A(1)), ('fwd', 2, A(1), None, A(2))]
HOOK3 = [('hook', 'x', As(0, 2))]
TANH_HEAD = [('act_bwd', DY, A(2), 'tanh', DLAST)]
# name: (record_step arguments, the sequence, the host queries) -- recorded like VDSR-5's, before the planners existed
FURTHER = {
    'srcnn': (dict(specs=SRCNN_SPECS(), x_shape=(4, 33, 33, 3), loss_kind='rownorm'),
              FWD3 + [('rownorm', A(2), 'hd', DY, ('rownorms',))] + TANH_HEAD + small_backward('srcnn'), (4, 0, 3, 0)),
    'espcn_one_launch_forward': (dict(specs=ESPCN_SPECS(), x_shape=(4, 17, 17, 3), hook=True),
                                 HOOK3 + [('mse', A(2), 'hd', DY)] + small_backward('espcn'), (0, 0, 3, 0)),
    'espcn_hook_declines': (dict(specs=ESPCN_SPECS(), x_shape=(4, 17, 17, 3), hook=False),
                            HOOK3 + FWD3 + [('mse', A(2), 'hd', DY)] + small_backward('espcn'), (3, 0, 3, 0)),
    'tanh_last_layer': (dict(specs=TANH3_SPECS(), x_shape=(2, 9, 9, 3)),
                        FWD3 + [('mse', A(2), 'hd', DY)] + TANH_HEAD + small_backward('tanh3'), (3, 0, 3, 0)),
}


@pytest.mark.parametrize('name', sorted(FURTHER))
def test_further_step_sequences(monkeypatch, name):
    args, sequence, parent_queries = FURTHER[name]
    events, queries = record_step(monkeypatch, **args)
    assert events == sequence
    assert_no_more_queries(queries, parent_queries)


def test_forty_body_layers_hit_every_cap_of_32(monkeypatch):
    """Both library predicates faked to yes: two forward chains (32 + 8 layers), ONE data-gradient chain of the 32 layers
    below the last one, ONE filter-gradient batch of the first 32 body layers; what is left of each runs per layer."""
    monkeypatch.setattr(ops, 'chain_supported', lambda *args, **kwargs: True)
    monkeypatch.setattr(ops, 'bwd_filter_batch_plan', lambda *args, **kwargs: (1, 256))
    events, queries = record_step(monkeypatch, DEEP_SPECS(), (1, 8, 8, 3))
    DX1, DX2 = ('dx', 1, 64), ('dx', 2, 64)
    assert events == (
        [('fwd', 0, 'x', None, A(0)),
         ('fwd_chain', list(range(1, 33)), As(0, 31), As(1, 32)),
         ('fwd_chain', list(range(33, 41)), As(32, 39), As(33, 40)),
         ('fwd', 41, A(40), None, A(41)),
         ('mse', A(41), 'hd', DY),
         ('wgrad', 41, A(40), DY),
         ('dgrad', 41, DY, A(40), 'relu', DX2),
         ('dgrad_chain', list(range(40, 8, -1)), [DX2] + Cs(9, 39)[::-1], As(8, 39)[::-1], 'relu', Cs(8, 39)[::-1]),
         ('wgrad', 40, A(39), DX2)] +
        [('wgrad', i, A(i - 1), C(i)) for i in range(39, 32, -1)] +
        [('dgrad', i, C(i), A(i - 1), 'relu', C(i - 1)) for i in range(8, 1, -1)] +
        [('wgrad_batch', list(range(1, 33)), As(0, 31), Cs(1, 32)),
         ('dgrad', 1, C(1), A(0), 'relu', DX1),
         ('wgrad', 0, 'x', DX1)])
    assert_no_more_queries(queries, (74, 1, 42, 1))


def test_vdsr20_queries_per_step(monkeypatch, switches):
    """(c) at the benchmark's shape: 37 chain queries (19 forward, 18 data gradient), one batch plan, 20 + 1 workspace sizes."""
    switches(1, 1)
    events, queries = record_step(monkeypatch, model_vdsr.layer_specs(20), (256, 41, 41, 3), residual=True, weight_decay=1e-4)
    assert [e[0] for e in events] == ['fwd', 'fwd_chain', 'fwd', 'mse', 'l2', 'wgrad', 'dgrad', 'dgrad_chain', 'wgrad_batch', 'wgrad']
    assert_no_more_queries(queries, (37, 1, 20, 1))


# ---- (b) the planners against the real library: VDSR, residual, host queries only -----------------------------------
def check_dataflow(bwd, specs):
    """Walks a backward plan with `holds[key]` = the layer whose output gradient the buffer holds at that point: every op
    must find the gradient of ITS layer under the key it reads (so no rotating buffer was overwritten too early), and
    every layer gets exactly one filter gradient and every layer but 0 one data gradient."""
    last = len(specs) - 1
    holds = {('dy', 0) if specs[last].act is None else ('dpre_last',): last}
    wgrads, dgrads = [], []
    for op in bwd:
        kind = type(op)
        if kind is engine.Wgrad:
            assert holds[op.dpre_key] == op.i
            wgrads.append(op.i)
        elif kind is engine.WgradBatch:
            assert [holds[key] for key in op.dpre_keys] == list(range(op.lo, op.hi + 1))
            wgrads += range(op.lo, op.hi + 1)
        elif kind is engine.Dgrad:
            assert holds[op.src_key] == op.i
            holds[op.dst_key] = op.i - 1
            dgrads.append(op.i)
        else:
            assert kind is engine.DgradChain and holds[op.src_key] == op.hi and len(op.dst_keys) == op.hi - op.lo + 1
            assert len(set(op.dst_keys) | {op.src_key}) == len(op.dst_keys) + 1        # (one launch: every layer another buffer)
            for k, key in zip(range(op.hi, op.lo - 1, -1), op.dst_keys):
                holds[key] = k - 1
                dgrads.append(k)
    assert sorted(wgrads) == list(range(last + 1)) and dgrads == list(range(last, 0, -1))


def runs_of(plan, kind):
    return [(op.lo, op.hi) for op in plan if type(op) is kind]


def vdsr_groupings(num_layers, x_shape, precision='highest'):
    """(forward chains, data-gradient chains, filter-gradient batches) of VDSR-num_layers, as inclusive (lo, hi) runs."""
    stack = ConvStack(model_vdsr.layer_specs(num_layers), device='cpu', residual=True, weight_decay=1e-4, precision=precision)
    args = (stack.specs, stack.residual, stack.layer_precision, [tuple(x_shape)] + stack._shapes(x_shape))
    fwd, bwd = engine.plan_forward(*args), engine.plan_backward(*args)
    assert (fwd, bwd) == (engine.plan_forward(*args), engine.plan_backward(*args))          # plans are data: they compare with ==
    assert [i for op in fwd for i in ([op.i] if type(op) is engine.Conv else range(op.lo, op.hi + 1))] == list(range(num_layers))
    check_dataflow(bwd, stack.specs)
    return runs_of(fwd, engine.Chain), runs_of(bwd, engine.DgradChain), runs_of(bwd, engine.WgradBatch)


BENCH = (256, 41, 41, 3)
BODY = [(1, 18)]


@pytest.fixture
def L():
    lib = _lib.lib()
    try:
        lib.srx_set_chain(1)
        lib.srx_set_wgrad_batch(1)
        yield lib
    finally:
        lib.srx_set_chain(-1)
        lib.srx_set_wgrad_batch(-1)
        lib.srx_set_wgrad_path(-1)
        lib.srx_set_conv_path(1)


@pytest.mark.parametrize('x_shape,precision,expected', [
    (BENCH, 'highest', (BODY, BODY, BODY)),
    ((64, 41, 41, 3), 'highest', ([], [], BODY)),        # a chain wants N to be a multiple of the 256-workgroup grid
    ((255, 41, 41, 3), 'highest', ([], [], BODY)),
    ((256, 42, 42, 3), 'highest', (BODY, BODY, [])),     # the batched filter gradient is the 41-pixel-row kernel's
    (BENCH, 'high', ([], [], [])),                       # bf16x3 body layers: neither grouping
])
def test_vdsr20_groupings_by_shape_and_precision(L, x_shape, precision, expected):
    assert vdsr_groupings(20, x_shape, precision) == expected


@pytest.mark.parametrize('switch,value,expected', [
    ('srx_set_chain', 0, ([], [], BODY)),
    ('srx_set_wgrad_batch', 0, (BODY, BODY, [])),
    ('srx_set_wgrad_path', 0, (BODY, BODY, [])),
    ('srx_set_wgrad_path', 1, (BODY, BODY, [])),
    ('srx_set_conv_path', 0, ([], [], BODY)),
])
def test_vdsr20_groupings_follow_the_switches_between_two_calls(L, switch, value, expected):
    assert vdsr_groupings(20, BENCH) == (BODY, BODY, BODY)
    getattr(L, switch)(value)
    assert vdsr_groupings(20, BENCH) == expected            # (nothing is cached: the next plan sees the switch)


def test_short_vdsr_stacks(L):
    assert vdsr_groupings(3, BENCH) == ([], [], [])         # one body layer: no run of two
    assert vdsr_groupings(4, BENCH) == ([(1, 2)], [(1, 2)], [(1, 2)])


def test_fake_predicates_cap_every_run_at_32():
    specs = DEEP_SPECS()
    shapes = [(1, 8, 8, 3)] + [(1, 8, 8, s.cout) for s in specs]
    asked = []
    yes = dict(chain_ok=lambda i, in_shape, op: True, batch_ok=lambda lo, hi: asked.append((lo, hi)) or True)
    fwd = engine.plan_forward(specs, False, ['highest'] * 42, shapes, chain_ok=yes['chain_ok'])
    bwd = engine.plan_backward(specs, False, ['highest'] * 42, shapes, **yes)
    assert fwd == [engine.Conv(0), engine.Chain(1, 32), engine.Chain(33, 40), engine.Conv(41)]
    assert runs_of(bwd, engine.DgradChain) == [(9, 40)] and runs_of(bwd, engine.WgradBatch) == [(1, 32)] and asked == [(1, 32)]
    assert engine.RUN_MAX == 32
    check_dataflow(bwd, specs)
    no = dict(chain_ok=lambda i, in_shape, op: False, batch_ok=lambda lo, hi: False)
    assert engine.plan_forward(specs, False, ['highest'] * 42, shapes, chain_ok=no['chain_ok']) == [engine.Conv(i) for i in range(42)]
    per_layer = engine.plan_backward(specs, False, ['highest'] * 42, shapes, **no)
    assert [type(op) for op in per_layer] == [engine.Wgrad, engine.Dgrad] * 41 + [engine.Wgrad]
    check_dataflow(per_layer, specs)

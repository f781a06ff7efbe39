"""engine.capture_graph keeps Python's cyclic collector out of a stream capture (no GPU needed).

A model and its ConvStack refer to each other, so a dropped model is freed by the cyclic collector; if that happened while a
stream captures, the graphs and memory pools the model owns would be released inside the capture, which aborts the process.
"""
import contextlib
import gc

import pytest
import torch

from ml_super_resolution_amd import engine


class _Node(object):
    def __init__(self, log):
        self.me = self          # a cycle: only the collector frees it
        self.log = log

    def __del__(self):
        self.log.append(gc.isenabled())


@pytest.fixture
def fake_graph(monkeypatch):
    state = {'inside': False, 'freed_inside': []}

    @contextlib.contextmanager
    def fake(g):
        state['inside'] = True
        try:
            yield
        finally:
            state['inside'] = False
    monkeypatch.setattr(torch.cuda, 'graph', fake)
    return state


def test_dead_cycles_are_collected_before_the_capture_and_none_during_it(fake_graph):
    assert gc.isenabled()
    log = []
    _Node(log)
    seen = {}
    with engine.capture_graph(object()):
        seen['before'] = list(log)
        assert fake_graph['inside']
        assert not gc.isenabled()
        _Node(log)
        # enough allocations to pass every generation's threshold many times over
        junk = [[i] for i in range(200000)]
        del junk
        seen['during'] = list(log)
    assert len(seen['before']) == 1, 'the cycle that was dead before the capture must be gone when it starts'
    assert seen['during'] == seen['before'], 'nothing may be collected while the stream captures'
    assert gc.isenabled()
    gc.collect()
    assert len(log) == 2


def test_collector_state_is_restored(fake_graph):
    gc.disable()
    try:
        with engine.capture_graph(object()):
            assert not gc.isenabled()
        assert not gc.isenabled(), 'a collector the caller had switched off stays off'
    finally:
        gc.enable()
    with pytest.raises(RuntimeError):
        with engine.capture_graph(object()):
            raise RuntimeError('launch failed')
    assert gc.isenabled(), 'an error inside the capture must not leave the collector off'

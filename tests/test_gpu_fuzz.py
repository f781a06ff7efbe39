"""Random layer shapes (both kernel families): forward, masked dgrad and wgrad through the C ABI against the oracle -- on
random floats within the tolerances, and on small integers exactly."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu


def _fuzz():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts', 'fuzz_conv.py')
    spec = importlib.util.spec_from_file_location('fuzz_conv', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('path', [1, 0], ids=['pipelined', 'two_wg_per_cu'])
def test_random_shapes_vs_oracle(path):
    from ml_super_resolution_amd import _lib
    old = _lib.lib().srx_set_conv_path(path)
    try:
        failures = _fuzz().run(60, 1000 + path, verbose=False)
    finally:
        _lib.lib().srx_set_conv_path(old)
    assert not failures, failures[:5]


@pytest.mark.parametrize('path', [1, 0], ids=['pipelined', 'two_wg_per_cu'])
def test_random_shapes_equal_the_oracle_on_integers(path):
    """The same shape generator on integer operands (scripts/fuzz_conv.py, run_integers): every result EQUALS the float64
    oracle; seeds of its own."""
    from ml_super_resolution_amd import _lib
    old = _lib.lib().srx_set_conv_path(path)
    fuzz = _fuzz()
    try:
        failures = fuzz.run(60, 2000 + path, verbose=False, integers=True)
    finally:
        _lib.lib().srx_set_conv_path(old)
    print('integer sweep, conv path %d: %d comparisons, largest magnitude / 2^24 = %.4f' % (path, fuzz.INT_STATS['checks'], fuzz.INT_STATS['magnitude']))
    assert not failures, failures[:5]
    assert fuzz.INT_STATS['checks'] >= 5 * 60 and fuzz.INT_STATS['magnitude'] < 1.0

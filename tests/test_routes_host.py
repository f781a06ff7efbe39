"""Which kernel every convolution runs on, and with which launch arguments, pinned on the host: a CPU test.

tests/route_trace_driver.cpp is linked with a plain --cuda-host-only build of srx_api.hip (no device code, no
sanitizer) and launcher stubs that write down every offer: launcher, key, grid, LDS bytes, min_pixels and every
field of the argument struct.  It runs ~900 shapes -- every model's layers, the widths / channel counts / sizes around
every threshold of a route predicate, every epilogue form, chains, batches, blocked pairs, precision 1, every runtime
switch -- under every acceptance mask, with 256 and 24 CUs and with each environment knob in its non-default state.

tests/golden/conv_routes.txt holds one line per group of cases (a tag and an entry point, "width/wgrad"): the 64-bit hash
of the group's output under all 18 configurations, then four digits of each case's own hash, which name the case that moved.
A refactoring of srx_api.hip leaves it as it is.  An intended route change shows up as changed lines; to re-record,
build the driver as this test does and run

    route_trace_driver --record > tests/golden/conv_routes.txt

(`route_trace_driver --case NAME` prints one case in full; set the knob in the environment, or ROUTE_TRACE_CUS=24, to
see it under another configuration).  DESIGN.md section 3.24 says how to read a trace."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_routes.txt')
HIPCC = '/opt/rocm/bin/hipcc'
# N, H, W, Cin, Cout, K, padding of tests/test_gpu_enet_pat.py::test_generic_kernel_with_a_tile_above_64_kib
GENERIC_ABOVE_64K = (16, 68, 24, 64, 16, 7, 'same')


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('routes') / 'route_trace_driver')
    csrc = os.path.join(ROOT, 'ml_super_resolution_amd', 'csrc')
    cmd = [HIPCC, '-O1', '-std=c++17', '--cuda-host-only', '--offload-arch=gfx950', '-Wl,--as-needed', '-Wno-unused-result',
           os.path.join(csrc, 'srx_api.hip'), '-x', 'hip', os.path.join(ROOT, 'tests', 'route_trace_driver.cpp'), '-o', exe]
    build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode(errors='replace')[-4000:]
    return exe


def _run(args, env=None):
    run = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
    out = run.stdout.decode(errors='replace')
    assert run.returncode == 0, out[-4000:]
    return out


def _clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith('SRX_') and k != 'ROUTE_TRACE_CUS'}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_conv_routes_match_the_golden(driver):
    """Every case's launcher offers and arguments, under every mask and configuration, hash to the recorded value."""
    env = _clean_env()
    got = [l for l in _run([driver, '--record'], env).splitlines() if not l.startswith('#')]
    with open(GOLDEN) as f:
        want = [l for l in f.read().splitlines() if not l.startswith('#')]
    assert len(want) > 50 and sum(len(l.split(':')[1].split()) for l in want) > 900
    if got == want:
        return
    # the cases whose digits moved: the k-th digits of a group belong to its k-th case in the order of --hashes
    names = {}
    for line in _run([driver, '--hashes'], env).splitlines():
        tag, rest = line.split(' ')[0].split('/', 1)
        names.setdefault(tag + '/' + re.split('[/_+]', rest)[0], []).append(line.split(' ')[0])
    want_by_group = {l.split(' ')[0]: l.split(':')[1].split() for l in want}
    changed = []
    for line in got:
        group, digits = line.split(' ')[0], line.split(':')[1].split()
        old = want_by_group.get(group, [])
        changed += [n for k, n in enumerate(names[group]) if k >= len(old) or len(old) != len(digits) or old[k] != digits[k]]
    report = ['golden lines differ: %s; %d cases moved, the first ones in full under the default configuration (a case that reads '
              'the same there differs under a knob or at 24 CUs):' % (sorted(set(got) ^ set(want))[:6], len(changed))]
    for case in changed[:3]:
        report.append('#### %s\n%s' % (case, _run([driver, '--case', case], env)))
    pytest.fail('\n'.join(report)[:20000])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_the_sweep_reaches_every_launcher(driver):
    """The cases offer a shape to every launcher stub at least once, and every one accepts at least once."""
    out = _run([driver, '--coverage'], _clean_env())
    print(out)
    rows = [l.split() for l in out.splitlines() if l.startswith('launch_')]
    assert len(rows) == 33, out
    for name, _, offered, _, accepted in rows:
        assert int(offered) >= 1 and int(accepted) >= 1, (name, offered, accepted)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')
def test_the_generic_kernel_gpu_case_is_planned_above_64_kib(driver):
    """The shape of test_generic_kernel_with_a_tile_above_64_kib is there to launch conv_mfma_generic_kernel with more than
    64 KiB of dynamic LDS (256 CUs).  Its key, 7x7 from 64 channels to one chunk, is in no tuned instance list, so on the
    device every launcher before launch_conv_generic refuses it; the planner's tile decides the bytes, and a planner change
    that takes the case below 64 KiB fails here.  (`route_trace_driver --fwd 16 68 24 64 16 7 0` prints the trace.)"""
    n, h, w, cin, cout, k, pad = GENERIC_ABOVE_64K
    out = _run([driver, '--fwd'] + [str(v) for v in (n, h, w, cin, cout, k, {'same': 0, 'valid': 1}[pad])], _clean_env())
    offers = re.findall(r'launch_conv_generic key=7,7,64,1,0 grid=\d+ lds=(\d+) ', out)
    assert offers and min(int(b) for b in offers) > 64 * 1024, out[:4000]      # (75,072: 4-row tiles, 27-slot rows)

"""The rule of csrc/lds_launch.h -- a kernel's dynamic-LDS ceiling is raised once per kernel instance, device and
thread -- checked on the CPU: tests/lds_limit_driver.cpp defines the two HIP runtime calls the rule makes, records them,
and calls raise_lds_limit with plain host functions as the kernels, so nothing is launched and no HIP runtime starts."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')
@pytest.mark.parametrize('sanitize', [(), ('-fsanitize=thread', '-fno-gpu-sanitize')], ids=['plain', 'tsan'])
def test_lds_limit_is_raised_once_per_kernel_device_and_thread(tmp_path, sanitize):
    """One call of 160 KiB per kernel and device; a second device and a second kernel of the same signature get their
    own; a failing hipFuncSetAttribute or hipGetDevice is returned and not remembered; device 64 is set on each call
    and leaves 0..63 alone; two threads each raise for themselves (and, built with ThreadSanitizer, share no state)."""
    exe = str(tmp_path / 'lds_limit')
    cmd = ['/opt/rocm/bin/hipcc', '-O1', '-g', '-std=c++17', *sanitize, '--cuda-host-only', '--offload-arch=gfx950',
           '-Wl,--as-needed',          # (nothing left to take from libamdhip64: not even loaded)
           '-Wall', '-x', 'hip', os.path.join(ROOT, 'tests', 'lds_limit_driver.cpp'), '-o', exe, '-lpthread']
    build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode(errors='replace')[-4000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                         env=dict(os.environ, TSAN_OPTIONS='halt_on_error=1 exitcode=66'))
    out = run.stdout.decode(errors='replace')
    assert run.returncode == 0 and 'ThreadSanitizer' not in out and 'lds limit driver ok' in out, out[-4000:]

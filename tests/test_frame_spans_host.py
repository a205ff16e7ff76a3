"""The host helpers every frame-level entry point shares (poccala_amd/csrc/frame_spans.h: the span and speaker checks, the upload, the
chunk plan and its one packed list, the check and upload of a label per frame row, the environment reader), without a GPU: tests/frame_spans_host_check.cpp is compiled against a stub context and a malloc-backed
stub pool with the host's address and undefined-behaviour sanitizers and run as a process of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def test_span_helpers_under_the_host_sanitizers(tmp_path):
    if not os.path.exists(HIPCC) and not shutil.which('hipcc'):
        pytest.fail('hipcc is needed to build the check (it is what builds the library)')
    exe = str(tmp_path / 'frame_spans_host_check')
    cmd = [HIPCC if os.path.exists(HIPCC) else 'hipcc', '--offload-arch=gfx950', '-std=c++17', '-g', '-O1', '-fno-omit-frame-pointer',
           '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
           os.path.join(ROOT, 'tests', 'frame_spans_host_check.cpp'), '-o', exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'frame_spans_host_check: OK' in run.stdout
    assert 'ERROR: AddressSanitizer' not in run.stderr and 'runtime error' not in run.stderr, run.stderr

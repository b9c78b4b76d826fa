"""The launch layer's (device id, slot) table (csrc/tg_launch.h) driven by a host-only program: the table makes no HIP
call, so tests/launch_table_check.cpp includes the header without hipcc and passes counting fake actions.  Built here
with the host compiler, the way tests/test_oracle_c.py builds the C oracle.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'tecogan-pytorch_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'launch_table_check.cpp')


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path_factory.mktemp('launch_table') / 'launch_table_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-pthread', '-I', CSRC, SRC, '-o', exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return p.returncode, p.stdout + p.stderr


@pytest.mark.parametrize('check', ['once_per_device_and_slot', 'failure_is_not_recorded', 'out_of_range_is_never_cached',
                                   'eight_threads_one_slot'])
def test_launch_table(report, check):
    """once_per_device_and_slot: the action runs exactly once per (device, slot) for devices 0 and 1, in either order;
    failure_is_not_recorded: a failing action is not recorded as done and runs again on the next call;
    out_of_range_is_never_cached: a device id outside the table is never cached and never indexes out of bounds;
    eight_threads_one_slot: eight threads hammering one slot run the action once."""
    rc, out = report
    assert f'ok {check}' in out.splitlines(), out


def test_launch_table_program_passes_as_a_whole(report):
    rc, out = report
    assert rc == 0 and 'FAILED' not in out, out

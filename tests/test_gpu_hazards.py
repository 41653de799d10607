"""Systematic screen of the hand-placed LDS-DMA waits: a diagnostic build (-DCR_POISON) overwrites every LDS piece
with bf16 NaNs right before it is refilled -- the point from which, by the schedules' own WAR / RAW rules, nobody may read it until the new bytes
have landed.  A read that breaks either rule then returns NaNs, so the integer-exact / bit-exact kernel tests FAIL on such a build instead of passing
whenever the old bytes happen to be still (or the new ones already) there.  This test builds that variant of gemm256.hip (both schedules) and
attention_vit.hip and runs the kernel tests on it in a child process; a second test shows that the screen has teeth: with the cold-start wait and
every counted wait of the main loop taken out (-DCR_BREAK_WAIT) the poisoned build returns NaNs on every shape of scripts/hazard_teeth.py -- the
plain build with the same break returns wrong numbers on most shapes and, run to run, the RIGHT ones on some (the race the screen exists for).
What the screen cannot see, measured the same way: with only the main loop's counted waits removed every shape still passes, poisoned or not,
under a copy hog on a second stream -- a staged piece has three phases (~1 us) to land and always does; those waits are correct by construction
(HISTORY.md, round 4), not by test."""
import json
import os
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_tests_pass_on_the_poisoned_build():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip('hipcc is not on this box: the diagnostic variant cannot be built')
    env = dict(os.environ, PATH=os.environ.get('PATH', '') + ':/opt/rocm/bin')
    b = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'build_variant.py'), 'poison', 'gemm256.hip,attention_vit.hip', '-DCR_POISON=1'],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    lib = os.path.join(ROOT, 'ab', 'libpoison.so')
    assert os.path.exists(lib)
    sel = 'gemm256 or gemm_epilogues or gelu or both_schedules or back_to_back or attention_vit or patch_rows or swiglu or argmax or tail_rows'
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.join(ROOT, 'tests', 'test_gpu_ops.py'), os.path.join(ROOT, 'tests', 'test_gpu_vit_attention.py'),
                        '-x', '-q', '-m', 'gpu', '-k', sel],
                       capture_output=True, text=True, env=dict(env, CR_HIP_LIB=lib), cwd=ROOT, timeout=900)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail
    assert ' passed' in tail and 'failed' not in tail, tail


def test_the_screen_sees_a_broken_schedule():
    if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
        pytest.skip('hipcc is not on this box: the diagnostic variant cannot be built')
    env = dict(os.environ, PATH=os.environ.get('PATH', '') + ':/opt/rocm/bin')
    b = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'build_variant.py'), 'poisonbroken', 'gemm256.hip', '-DCR_POISON=1', '-DCR_BREAK_WAIT=1'],
                       capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    lib = os.path.join(ROOT, 'ab', 'libpoisonbroken.so')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'hazard_teeth.py')], capture_output=True, text=True,
                       env=dict(env, CR_HIP_LIB=lib, CR_TEETH_ITERS='2'), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert res['lib'] == lib
    for case in res['cases']:
        assert case['nan'] > 0, case                          # the unlanded piece was read as NaNs, on both schedules

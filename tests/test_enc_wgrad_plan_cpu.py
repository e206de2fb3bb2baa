"""The contraction plan of the encoder LSTMs' live-row weight gradients (visdial_amd/csrc/wgrad_plan.h) is host code without a HIP
type: tests/enc_wgrad_plan_check.cpp is a stand-alone program around it, built here with the host compiler under
-fsanitize=address,undefined and run.  For N in {1, 15, 16, 17, 40, 200} rows per step, T in {1, 2, 7, 40} steps and non-decreasing
live-row counts (random; with leading zeros = no row of full length; drawn from {0, 1, 15, 16, 17, N}; all N) it walks every work list the
way the kernel does and checks that
  * every live (t, i) pair is contracted exactly once per product and output tile, a pad pair at most once;
  * no k-step reads a row of another step, and a row taken in beyond nact[t] lies in [nact[t], N) of the same step;
  * the chunks (one workgroup's share) differ by at most one k-step, for 1, 5, 64 and 768 chunks;
  * the dWh products pair the h row (t - 1, i) with the da row (t, i), and step 0 has no pair."""
import os
import subprocess

from conftest import ROOT


def test_plan_covers_the_live_pairs_once_inside_their_steps(tmp_path):
    exe = str(tmp_path / 'enc_wgrad_plan_check')
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                        '-I', os.path.join(ROOT, 'visdial_amd', 'csrc'), os.path.join(ROOT, 'tests', 'enc_wgrad_plan_check.cpp'), '-o', exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith('OK '), r.stdout

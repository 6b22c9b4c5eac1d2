"""Stage timing of the generated instance kernel (config 2's per-instance phase) from inside: debug_stage 20 makes every
handed-over instance write the 100 MHz time stamps of its stages over its first primal results; debug_stage 24 adds two
stamps inside the factorisation stage (factorised: LDL' and block inverses; coefficients in registers; the stage's own
stamp then closes the slice restore).  Only eight stamps are kept, and in the single-kernel step the in-loop
factorisation falls behind the eighth: placement 4 (two kernels) makes the instance kernel factor at its start, with the
same generated function.
    python scripts/gpu_probe_instance.py [B] [json settings] [placement] [split]"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from cvxpygen_amd import families
from cvxpygen_amd.runtime import BatchSolver, build_family_plan

B = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
stg = json.loads(sys.argv[2]) if len(sys.argv) > 2 else {}
placement = int(sys.argv[3]) if len(sys.argv) > 3 else None
split = len(sys.argv) > 4 and sys.argv[4] == 'split'
d = families.mpc(12, 4, 10)
plan = build_family_plan(d)
lib = os.path.join(ROOT, 'cvxpygen_amd', 'generated', 'mpc12', os.environ.get('CPG_PROBE_LIB', 'libcpg_mpc12.so'))
bs = BatchSolver(d, lib_path=lib, plan=plan)
if placement is not None:
    bs.set_program_placement(placement)
bs.set_updated(['x_init'])
th = bench.make_theta(d, B, seed=1000)
r0 = bs.solve(theta_var=th, **stg)
r = bs.solve(theta_var=th, debug_stage=24 if split else 20, **stg)
ho = r0.iter > 50
print('instances', B, 'handed over', int(ho.sum()), 'mean iter', r0.iter.mean(), 'phase ms', bs.last_phase_ms())
ts = r.prim_flat[ho][:, :8] * 0.01            # microseconds since the instance started in the instance kernel
names = ['start', 'classes', 'factor', 'state', 'iterate', 'check', 'iterate2/final', 'check2/final', '...']
if split:
    names = ['start', 'classes', 'factor: LDL\' + inverses', 'factor: coefficients', 'factor: slice restore', 'state', 'iterate', 'check', '...']
one = ts[(r0.iter[ho] == 75)]
print('instances that finish at the test of iteration 75:', len(one))
d_ = np.diff(one[:, :8 if split else 7], axis=1)
for k in range(d_.shape[1]):
    print(f'  {names[k + 1]:26s} mean {d_[:, k].mean():9.1f} us   median {np.median(d_[:, k]):9.1f}   p90 {np.percentile(d_[:, k], 90):9.1f}')
if split:
    print(f'  factor (the three together) mean {(one[:, 4] - one[:, 1]).mean():9.1f} us')
else:
    print('  total per instance (mean)', one[:, 6].mean() if one.shape[1] > 6 else None)

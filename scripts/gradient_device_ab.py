"""One training step -- forward solve + QP adjoint -- of BASELINE config 5 (MPC 12/4/10, x_init varying, upstream
dX = dU = 0.1, 20 000 instances) through the host entry points or through the device objects; the numbers behind
profiles/gradient_device_ab.txt.

    python scripts/gradient_device_ab.py --mode host   [--batch 20000 --steps 20 --warmup 5]
    python scripts/gradient_device_ab.py --mode device

host:    BatchSolver.solve + BatchSolver.gradient: theta, the solution, the canonical dx up and the results down on every step
         (runs on any commit that has the adjoint).
device:  solve_device + gradient_device on a DeviceBatch / DeviceGradBatch, the adjoint ordered behind the solve by an event,
         one synchronisation of the gradient handle per step.  `device_io` adds what a caller whose parameters and
         loss live on the host still pays: theta_var up before the step, dtheta down after it.
Prints one JSON line: ms per step (mean of the timed steps), the adjoint kernel's own time, and a checksum of dtheta."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvxpygen_amd import codegen, families            # noqa: E402
from cvxpygen_amd import runtime as rt                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=['host', 'device'], required=True)
    ap.add_argument('--batch', type=int, default=20000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--dump', default=None, metavar='FILE', help='write dtheta [B][NP] of the last step as .npy')
    args = ap.parse_args()
    B = args.batch
    desc = families.mpc(12, 4, 10)
    plan = rt.build_family_plan(desc)
    lib = codegen.build_family_library(plan, os.path.join(ROOT, 'cvxpygen_amd', 'generated', 'mpc12'), 'mpc12')
    gs = rt.BatchSolver(desc, lib_path=lib, full_output=True, plan=plan)
    x0 = -2.0 + 4.0 * np.random.default_rng(77).random((B, 12))
    dv = {v.name: np.full((B,) + tuple(v.shape), 0.1) for v in desc.variables}
    out = {'mode': args.mode, 'instances': B, 'steps': args.steps, 'warmup': args.warmup}

    def kernel_ms():
        ms = rt.C.c_float(0)
        gs.lib.check(gs.lib.L.cpg_hip_last_kernel_ms(gs.h_grad, rt.C.byref(ms)), 'cpg_hip_last_kernel_ms')
        return float(ms.value)

    def timed(step):
        for _ in range(args.warmup):
            step()
        ts, ks = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            step()
            ts.append(time.perf_counter() - t0)
            ks.append(kernel_ms())
        return 1e3 * float(np.mean(ts)), float(np.mean(ks))

    if args.mode == 'host':
        last = {}

        def step():
            fw = gs.solve({'x_init': x0}, updated_params=['x_init'])
            last['g'] = gs.gradient({'x_init': x0}, fw.sol_x, fw.sol_y, dv, updated_params=['x_init'])
        out['ms_per_step'], out['adjoint_kernel_ms'] = timed(step)
        g = last['g']['_flat']
    else:
        gs.set_updated(['x_init'])
        gs.apply_settings()
        dev, gdev = rt.DeviceBatch(gs, B), rt.DeviceGradBatch(gs, B)
        tv = gs.theta_var({'x_init': x0})
        dev.upload(tv)
        gdev.upload_dvars(dv)

        def step():
            gs.solve_device(dev)
            gs.gradient_device(dev, gdev)
            gdev.synchronize()

        def step_io():
            dev.upload(tv)
            gs.solve_device(dev)
            gs.gradient_device(dev, gdev)
            gdev.download()
        out['ms_per_step'], out['adjoint_kernel_ms'] = timed(step)
        out['device_io'] = dict(zip(('ms_per_step', 'adjoint_kernel_ms'), timed(step_io)))
        g = gdev.download()['_flat']
        fw = dev.download()
        out['solved'] = int((fw.status == 1).sum())
        # the host entry point on the same solution: the two must agree bit for bit
        gh = gs.gradient({'x_init': x0}, fw.sol_x, fw.sol_y, dv, updated_params=['x_init'])['_flat']
        out['equals_host_entry_point'] = bool(np.array_equal(g, gh))
        dev.free(); gdev.free()
    if args.dump:
        np.save(args.dump, g)
    out['dtheta_abs_sum'] = float(np.abs(g).sum())
    out['dtheta_finite'] = bool(np.isfinite(g).all())
    gs.close()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()

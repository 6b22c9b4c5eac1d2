"""Single-kernel step of the default mode (rho adaptation on): the linked handle's generated instance kernel serves the
WHOLE batch in one launch, starting every instance from the family's coefficient table
(cpg_hip_set_instance_registers) instead of factoring, and refactoring in its loop where an instance's rho changes
(csrc/cpg_osqp_refactor.h, csrc/cpg_hip.cpp solve_shared; placement -1 picks it, 5 forces it, 1 keeps the two kernels).

CPU tier, on the lock-step emulator: parity with the two-kernel step (placement 1) and with the C oracle on a sample
that the oracle itself shows to hold every kind of instance, the guards of the table (row classes, rho / sigma stamp),
and the table against the device's own factorisation."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from cvxpygen_amd import families, resident_plan as rs
from cvxpygen_amd.runtime import BatchSolver, build_family_plan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def mpc6_lib(tmp_path_factory):
    from sim import build_sim
    d = families.mpc(6, 3, 10)
    plan = build_family_plan(d)
    out = str(tmp_path_factory.mktemp('single'))
    lib = build_sim.build_family(plan, out, 'mpc6')
    hdr = open(os.path.join(out, 'cpg_instance_mpc6.h')).read()
    assert '#define CPG_GENI_NNZX ' in hdr
    return d, plan, lib, int(re.search(r'#define CPG_GENI_NREGS (\d+)', hdr).group(1))


def _setting(bs, name):
    v = C.c_double(-1)
    bs.lib.check(bs.lib.L.cpg_hip_get_setting(bs.h_shared, name.encode(), C.byref(v)), 'get')
    return v.value


def _solver(d, plan, lib, placement):
    bs = BatchSolver(d, lib_path=lib, plan=plan)
    bs.set_launch(waves_per_block=2)
    bs.set_program_placement(placement)
    return bs


def _install(bs, plan, d, rho_stamp, garbage=False, sigma_stamp=None):
    """the family's table on the per-instance handle, stamped with rho_stamp / sigma_stamp (computed at the family's rho and
    sigma; garbage: 7.0 in every entry instead)"""
    from cvxpygen_amd.runtime import _Resident, _ip, _u16p, _i8p
    mg = bs._shared_mode_candidate().merged
    o = plan.osqp
    rho, sigma = float(o.settings['rho']), float(o.settings['sigma'])
    ct = np.ascontiguousarray(o.constr_type, dtype=np.int8)
    rho_vec = np.where(ct == 1, 1e3 * rho, np.where(ct == 0, rho, 1e-6))
    Ps, As = (plan.osqp_shared or o).pruned(d.P, d.A)
    coef = np.ascontiguousarray(rs.replay_solve_vals(mg, rs.replay_factor(mg, Ps.data, As.data, sigma, 1.0 / rho_vec)))
    if garbage:
        coef = np.full_like(coef, 7.0)
    ctab = np.ascontiguousarray(mg.sol.ctab, dtype=np.int32)
    dsc = np.ascontiguousarray(mg.sol.desc, dtype=np.uint32)
    cols = np.ascontiguousarray(mg.sol.cols, dtype=np.uint16)
    ms = _Resident(nnzX=mg.nnzX, sol_chunks=mg.sol.n_chunks, sol_nnz=mg.sol.nnz, sol_slots=mg.sol.n_slots,
                   sol_ctab=ctab.ctypes.data_as(_ip), sol_desc=dsc.ctypes.data_as(C.POINTER(C.c_uint32)),
                   sol_cols=cols.ctypes.data_as(_u16p))
    bs.lib.check(bs.lib.L.cpg_hip_set_instance_registers(bs.h_rs, C.byref(ms), coef.ctypes.data_as(C.POINTER(C.c_double)),
                                                        len(coef), ct.ctypes.data_as(_i8p), rho_stamp,
                                                        sigma if sigma_stamp is None else sigma_stamp),
                 'set_instance_registers')


def _sample():
    """seeded x_init of MPC 6/3/10 at six magnitudes: small ones terminate at the first test, large ones adapt rho"""
    rng = np.random.default_rng(0)
    return np.concatenate([s * (-1 + 2 * rng.random((8, 6))) for s in (0.02, 0.1, 0.3, 1.0, 2.0, 4.0)])


def test_single_kernel_parity_and_coverage(oracle_lib, mpc6_lib):
    """iteration counts and statuses identical to the two-kernel step and to the oracle, results within 1e-9 relative; the
    oracle ALONE shows that the sample holds instances that terminate before iteration 50, instances that adapt rho at 50
    and instances that pass 50 inside the tolerance band (cut off at iteration 74, before the next test, a solve with
    adaptation differs from one without exactly when rho changed at 50)"""
    from test_sim_kernel import _assert_parity, _oracle_flat, _theta
    d, plan, lib, _ = mpc6_lib
    v = _sample()
    th = _theta(d, 'x_init', v)
    o, prim, dual = _oracle_flat(oracle_lib, d, th, ['x_init'])
    o_ad = oracle_lib.cpg_solve_batch(d, th, ['x_init'], max_iter=74)
    o_fx = oracle_lib.cpg_solve_batch(d, th, ['x_init'], max_iter=74, adaptive_rho=0)
    early = o['iter'] < 50
    past = o['iter'] > 50
    in_band = past & (o_ad['sol_x'] == o_fx['sol_x']).all(axis=1) & (o_ad['sol_y'] == o_fx['sol_y']).all(axis=1)
    adapts = past & ~in_band
    assert early.any() and adapts.any() and in_band.any(), (early.sum(), adapts.sum(), in_band.sum())
    assert o['iter'].max() < 100           # (one adaptation event: the count below is of the instances that adapt at 50)
    res, phase = {}, {}
    for placement in (1, 5, -1):
        bs = _solver(d, plan, lib, placement)
        res[placement] = bs.solve({'x_init': v}, updated_params=['x_init'])
        assert _setting(bs, 'single_kernel_step') == (0.0 if placement == 1 else 1.0)
        phase[placement] = bs.last_phase_ms()
        bs.close()
    for placement in (5, -1):
        r, r1 = res[placement], res[1]
        _assert_parity(r, o, prim, dual)
        assert r.iter.tolist() == r1.iter.tolist() and r.status.tolist() == r1.status.tolist()
        for a, b in ((r.prim_flat, r1.prim_flat), (r.dual_flat, r1.dual_flat), (r.obj_val, r1.obj_val)):
            assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
        # one phase; its count is of the instances that refactored in the loop -- those the two-kernel step hands over
        assert phase[placement][0] > 0.0 and phase[placement][1] == 0.0
        assert phase[placement][2] == phase[1][2] == int(adapts.sum())
    assert phase[1][1] > 0.0


def test_other_settings_and_state(oracle_lib, mpc6_lib):
    """check_termination not aligned with the adaptation interval, tight tolerances (several adaptations), max_iter
    reached; a workspace that arrives with another rho than the family's factors on the device"""
    from test_sim_kernel import _assert_parity, _oracle_flat, _theta
    d, plan, lib, _ = mpc6_lib
    rng = np.random.default_rng(5)
    for B, stg in ((5, dict(check_termination=7, eps_abs=1e-6, eps_rel=1e-6)), (3, dict(max_iter=60))):
        v = -2 + 4 * rng.random((B, 6))
        o, prim, dual = _oracle_flat(oracle_lib, d, _theta(d, 'x_init', v), ['x_init'], **stg)
        bs = _solver(d, plan, lib, -1)
        r = bs.solve({'x_init': v}, updated_params=['x_init'], **stg)
        assert _setting(bs, 'single_kernel_step') == 1.0
        bs.close()
        _assert_parity(r, o, prim, dual)
    v0, v1 = -2 + 4 * rng.random((3, 6)), -2 + 4 * rng.random((3, 6))
    out = {}
    for placement in (5, 1):
        bs = _solver(d, plan, lib, placement)
        st = bs.solve({'x_init': v0}, updated_params=['x_init'], return_state=True).state.copy()
        st[1, -1] = 3.0 * st[1, -1]
        out[placement] = bs.solve({'x_init': v1}, updated_params=['x_init'], state_in=st, return_state=True)
        bs.close()
    assert out[5].iter.tolist() == out[1].iter.tolist() and out[5].status.tolist() == out[1].status.tolist()
    assert np.allclose(out[5].prim_flat, out[1].prim_flat, rtol=1e-9, atol=1e-11)
    assert np.allclose(out[5].state, out[1].state, rtol=1e-9, atol=1e-11)


def test_row_in_another_class_factors_on_the_device(oracle_lib, tmp_path):
    """an upper bound above the infinity threshold makes its row a free row: 1 / rho_vec of that instance differs from the
    family's, the table does not serve it -- it factors in the kernel and matches the oracle, next to instances that use
    the table.  (On toy_box, not on an MPC family: no parameter of the MPC families enters an inequality bound, so none of
    their instances can change a row's class; toy_box's library carries a merged instance program as well.)  The count of
    in-loop refactorisations holds the instances whose rho changed at iteration 50 -- which the oracle alone tells, as in
    test_single_kernel_parity_and_coverage -- and not the start-up factorisations of the free-row instances."""
    from sim import build_sim
    d = families.toy_box()
    plan = build_family_plan(d)
    lib = build_sim.build_family(plan, str(tmp_path), 'toy_box')
    assert '#define CPG_GENI_NNZX ' in open(os.path.join(str(tmp_path), 'cpg_instance_toy_box.h')).read()
    B = 6
    th = np.tile(d.theta0, (B, 1))
    ub = d.param('ub')
    th[1, ub.col] = 1e30
    th[3, ub.col] = np.inf
    th[4, d.param('a').col] = 4.0
    th[5, d.param('a').col] = 1000.0           # (adapts rho)
    th = np.clip(th, -1e30, 1e30)
    upd = ['a', 'lb', 'ub']
    tv = np.concatenate([th[:, d.param(nm).col:d.param(nm).col + d.param(nm).size] for nm in
                         [q.name for q in d.params if q.name in upd]], axis=1)
    o = oracle_lib.cpg_solve_batch(d, th, upd)
    bs = _solver(d, plan, lib, -1)
    r = bs.solve(updated_params=upd, theta_var=tv)
    assert _setting(bs, 'single_kernel_step') == 1.0
    count = bs.last_phase_ms()[2]
    bs.close()
    assert r.iter.tolist() == o['iter'].tolist() and r.status.tolist() == o['status'].tolist()
    o_ad = oracle_lib.cpg_solve_batch(d, th, upd, max_iter=74)
    o_fx = oracle_lib.cpg_solve_batch(d, th, upd, max_iter=74, adaptive_rho=0)
    adapts = (o['iter'] > 50) & ~((o_ad['sol_x'] == o_fx['sol_x']).all(axis=1) & (o_ad['sol_y'] == o_fx['sol_y']).all(axis=1))
    assert o['iter'].max() < 100 and adapts.any() and not adapts[[1, 3]].all()
    assert count == int(adapts.sum())
    ok = np.isin(o['status'], (1, 2, 7))
    sol = np.concatenate([o['sol_x'][:, v.indices] for v in d.variables], axis=1)
    assert np.abs(r.prim_flat[ok] - sol[ok]).max() <= 1e-9 * max(1.0, np.abs(sol[ok]).max())
    assert np.abs(r.obj_val[ok] - o['obj_val'][ok]).max() <= 1e-9 * max(1.0, np.abs(o['obj_val'][ok]).max())


@pytest.mark.parametrize('stale', ['rho', 'sigma'])
def test_stale_table_is_never_used(oracle_lib, mpc6_lib, stale):
    """a table stamped with another rho, or another sigma, than the handle's -- here one full of wrong numbers: -1 falls back
    to the two kernels and reports it, 5 refuses, the results are the oracle's; the table of the handle's rho and sigma
    restores the step"""
    from test_sim_kernel import _assert_parity, _oracle_flat, _theta
    d, plan, lib, _ = mpc6_lib
    v = _sample()[20:36]
    o, prim, dual = _oracle_flat(oracle_lib, d, _theta(d, 'x_init', v), ['x_init'])
    rho = float(plan.osqp.settings['rho'])
    bs = _solver(d, plan, lib, -1)
    bs.set_updated(['x_init'])
    assert _setting(bs, 'single_kernel_step') == 1.0
    sigma = float(plan.osqp.settings['sigma'])
    if stale == 'rho':
        _install(bs, plan, d, 2.0 * rho, garbage=True)
    else:
        _install(bs, plan, d, rho, garbage=True, sigma_stamp=2.0 * sigma)
    assert _setting(bs, 'single_kernel_step') == 0.0
    r = bs.solve(theta_var=v)
    _assert_parity(r, o, prim, dual)
    assert bs.last_phase_ms()[1] > 0.0            # (two kernels)
    # ... nor by the instance kernel itself when it is handed a whole batch at the family's rho (its own stamp tests: with
    # the rho stamp right and the sigma stamp wrong only the kernel's sigma test keeps the wrong numbers out)
    bs._apply_settings_to(bs.h_rs)
    sub = bs._solve_on(bs.h_rs, np.ascontiguousarray(v), len(v), None, False)
    assert sub[3].tolist() == o['iter'].tolist() and sub[4].tolist() == o['status'].tolist()
    assert np.abs(sub[0] - prim).max() <= 1e-9 * max(1.0, np.abs(prim).max())
    bs.set_program_placement(5)
    with pytest.raises(RuntimeError, match='single-kernel'):
        bs.solve(theta_var=v)
    _install(bs, plan, d, rho)
    assert _setting(bs, 'single_kernel_step') == 1.0
    r2 = bs.solve(theta_var=v)
    _assert_parity(r2, o, prim, dual)
    assert bs.last_phase_ms()[1] == 0.0
    bs.close()


def test_table_equals_the_device_factorisation(mpc6_lib):
    """what the fast path loads into the coefficient registers against what the kernel's own factorisation at the family's
    rho loads there (debug stage 21 writes register b mod NREGS of instance b over its first 64 primal results), to
    1e-12 relative -- of the table's largest entry and entry by entry (measured on the emulator: 8.9e-16 absolute at a
    largest entry of 100, 9.7e-16 entry by entry: both sides run the same dot-product schedule in double precision)"""
    d, plan, lib, nregs = mpc6_lib
    rho = float(plan.osqp.settings['rho'])
    bs = _solver(d, plan, lib, -1)
    bs.set_updated(['x_init'])
    v = np.tile(-2 + 4 * np.random.default_rng(3).random((1, 6)), (nregs, 1))
    bs._settings_kwargs = dict(debug_stage=21)
    bs._apply_settings_to(bs.h_rs)
    tab = bs._solve_on(bs.h_rs, v, nregs, None, False)[0][:, :64].copy()
    # the fast path is what ran: a recognisable table under the right stamp comes back as it is (7.0 on the lanes of
    # every step, 0.0 on idle lanes) -- a kernel that factored every instance would return the factor's numbers here
    _install(bs, plan, d, rho, garbage=True)
    seven = bs._solve_on(bs.h_rs, v, nregs, None, False)[0][:, :64].copy()
    assert np.isin(seven, (0.0, 7.0)).all() and (seven[tab != 0.0] == 7.0).all() and (seven == 7.0).sum() > 64     # (a step's coefficient may be 0.0)
    _install(bs, plan, d, 2.0 * rho)              # (stamp of another rho: the kernel factors)
    dev = bs._solve_on(bs.h_rs, v, nregs, None, False)[0][:, :64].copy()
    bs.close()
    assert np.isfinite(tab).all() and np.isfinite(dev).all()
    assert (tab != 0.0).sum() > 64 and ((tab == 0.0) == (dev == 0.0)).all()
    assert not np.array_equal(tab, np.zeros_like(tab))
    print('table vs device factorisation: max abs', np.abs(tab - dev).max(), 'max entry', np.abs(tab).max(),
          'max elementwise relative', (np.abs(tab - dev) / np.maximum(np.abs(tab), 1e-300)).max())
    assert np.abs(tab - dev).max() <= 1e-12 * np.abs(tab).max()
    assert (np.abs(tab - dev) <= 1e-12 * np.abs(tab)).all()

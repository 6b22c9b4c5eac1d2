"""Register executor of the shared-factor kernel (cpg_hip_set_shared_registers, placement 4 and the automatic choice): the
merged instance program of a family library, its coefficients from ONE host-side factorisation at the family's rho and
sigma, held in registers for the whole instance loop (csrc/cpg_osqp_kernel.h, osqp_shared_body<.., SharedRegExec>).

CPU tier, on the lock-step emulator: iteration counts and statuses against the C oracle AND against the LDS-resident
program of the same library (placement 1), the stamp check on rho / sigma, the setting that reports the executor."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from cvxpygen_amd import codegen, families, resident_plan as rs
from cvxpygen_amd.runtime import BUILD_OPTIONS_FIXED_RHO, BatchSolver, build_family_plan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def mpc6_lib(tmp_path_factory):
    from sim import build_sim
    d = families.mpc(6, 3, 10)
    plan = build_family_plan(d)
    out = str(tmp_path_factory.mktemp('sreg'))
    lib = build_sim.build_family(plan, out, 'mpc6')
    assert '#define CPG_GENI_NNZX ' in open(os.path.join(out, 'cpg_instance_mpc6.h')).read()
    return d, plan, lib


def _setting(bs, name):
    v = C.c_double(-1)
    bs.lib.check(bs.lib.L.cpg_hip_get_setting(bs.h_shared, name.encode(), C.byref(v)), 'get')
    return v.value


def _solver(d, plan, lib, placement, build_options=None):
    bs = BatchSolver(d, lib_path=lib, plan=plan, build_options=build_options or {})
    bs.set_launch(waves_per_block=2)          # (a batch of 5 leaves the last workgroup half empty)
    bs.set_program_placement(placement)
    return bs


def test_register_executor_parity(oracle_lib, mpc6_lib):
    """placement 4 against the oracle and against placement 1 of the same library: a batch that does not fill the last
    workgroup, check_termination not aligned with the adaptation interval, the fixed-rho fork (no per-instance handle:
    the table sits on the shared handle itself), max_iter reached; -1 picks the register executor, 1 does not"""
    from test_sim_kernel import _assert_parity, _oracle_flat, _theta
    d, plan, lib = mpc6_lib
    rng = np.random.default_rng(11)
    cases = [(5, {}, None), (3, dict(check_termination=7, eps_abs=1e-6, eps_rel=1e-6), None),
             (4, {}, dict(BUILD_OPTIONS_FIXED_RHO)), (3, dict(max_iter=30), None)]
    for B, stg, bo in cases:
        v = -2 + 4 * rng.random((B, 6))
        mode = dict(adaptive_rho=0, check_dualgap=0) if bo else {}
        o, prim, dual = _oracle_flat(oracle_lib, d, _theta(d, 'x_init', v), ['x_init'], **mode, **stg)
        res = {}
        for placement in (4, 1, -1):
            bs = _solver(d, plan, lib, placement, bo)
            res[placement] = bs.solve({'x_init': v}, updated_params=['x_init'], **stg)
            assert _setting(bs, 'register_executor') == (0.0 if placement == 1 else 1.0)
            bs.close()
        _assert_parity(res[4], o, prim, dual)
        for placement in (1, -1):
            r = res[placement]
            assert r.iter.tolist() == res[4].iter.tolist() and r.status.tolist() == res[4].status.tolist()
            ok = np.isin(r.status, (1, 2, 7))
            assert np.allclose(r.prim_flat[ok], res[4].prim_flat[ok], rtol=1e-9, atol=1e-11)
            assert np.allclose(r.dual_flat[ok], res[4].dual_flat[ok], rtol=1e-9, atol=1e-11)
        if 'max_iter' in stg:
            assert (res[4].status == 7).any()


def test_register_executor_state_in_with_another_rho(oracle_lib, mpc6_lib):
    """a workspace that arrives with another rho than the family's is handed over at iteration 0, as on the LDS program"""
    d, plan, lib = mpc6_lib
    rng = np.random.default_rng(12)
    v0, v1 = -2 + 4 * rng.random((3, 6)), -2 + 4 * rng.random((3, 6))
    out = {}
    for placement in (4, 1):
        bs = _solver(d, plan, lib, placement)
        r0 = bs.solve({'x_init': v0}, updated_params=['x_init'], return_state=True)
        st = r0.state.copy()
        st[1, -1] = 3.0 * st[1, -1]                # this one's rho is not the family's
        out[placement] = bs.solve({'x_init': v1}, updated_params=['x_init'], state_in=st)
        bs.close()
    assert out[4].iter.tolist() == out[1].iter.tolist() and out[4].status.tolist() == out[1].status.tolist()
    assert np.allclose(out[4].prim_flat, out[1].prim_flat, rtol=1e-9, atol=1e-11)


def test_stale_coefficients_are_never_used(mpc6_lib):
    """a table stamped with another rho than the handle's: -1 falls back to the LDS program, 4 refuses; installing the
    table for the handle's rho again restores the executor"""
    d, plan, lib = mpc6_lib
    v = -2 + 4 * np.random.default_rng(13).random((2, 6))
    bs = _solver(d, plan, lib, -1)
    r_reg = bs.solve({'x_init': v}, updated_params=['x_init'])
    assert _setting(bs, 'register_executor') == 1.0
    mg = bs._shared_mode_candidate().merged
    o = plan.osqp
    rho, sigma = float(o.settings['rho']), float(o.settings['sigma'])
    ct = np.asarray(o.constr_type)

    def install(rho_t):
        rho_vec = np.where(ct == 1, 1e3 * rho_t, np.where(ct == 0, rho_t, 1e-6))
        Ps, As = (plan.osqp_shared or o).pruned(d.P, d.A)
        coef = np.ascontiguousarray(rs.replay_solve_vals(mg, rs.replay_factor(mg, Ps.data, As.data, sigma, 1.0 / rho_vec)))
        from cvxpygen_amd.runtime import _Resident, _ip, _u16p
        ctab = np.ascontiguousarray(mg.sol.ctab, dtype=np.int32)
        dsc = np.ascontiguousarray(mg.sol.desc, dtype=np.uint32)
        cols = np.ascontiguousarray(mg.sol.cols, dtype=np.uint16)
        ms = _Resident(nnzX=mg.nnzX, sol_chunks=mg.sol.n_chunks, sol_nnz=mg.sol.nnz, sol_slots=mg.sol.n_slots,
                       sol_ctab=ctab.ctypes.data_as(_ip), sol_desc=dsc.ctypes.data_as(C.POINTER(C.c_uint32)),
                       sol_cols=cols.ctypes.data_as(_u16p))
        bs.lib.check(bs.lib.L.cpg_hip_set_shared_registers(bs.h_shared, C.byref(ms), coef.ctypes.data_as(C.POINTER(C.c_double)),
                                                          len(coef), rho_t, sigma), 'set_shared_registers')
    install(2.0 * rho)
    assert _setting(bs, 'register_executor') == 0.0
    r_lds = bs.solve({'x_init': v}, updated_params=['x_init'])
    assert r_lds.iter.tolist() == r_reg.iter.tolist() and r_lds.status.tolist() == r_reg.status.tolist()
    bs.set_program_placement(4)
    with pytest.raises(RuntimeError):
        bs.solve({'x_init': v}, updated_params=['x_init'])
    install(rho)
    assert _setting(bs, 'register_executor') == 1.0
    r2 = bs.solve({'x_init': v}, updated_params=['x_init'])
    assert np.array_equal(r2.prim_flat, r_reg.prim_flat) and r2.iter.tolist() == r_reg.iter.tolist()
    bs.close()


def test_library_without_merged_program_has_no_register_executor(tmp_path, monkeypatch):
    """a library whose instance header carries the plain program installs nothing: 4 refuses, -1 keeps the LDS program"""
    from sim import build_sim
    d = families.mpc(6, 3, 10)
    plan = build_family_plan(d)
    monkeypatch.setattr(rs, 'INSTANCE_MAX_GROUP_ROWS', 0)
    lib = build_sim.build_family(plan, str(tmp_path), 'mpc6')
    monkeypatch.undo()
    bs = _solver(d, plan, lib, 4, dict(BUILD_OPTIONS_FIXED_RHO))
    with pytest.raises(RuntimeError):
        bs.solve({'x_init': np.zeros((1, 6))}, updated_params=['x_init'])
    assert _setting(bs, 'register_executor') == 0.0
    bs.close()


def test_mpc12_register_executor_fits_the_lds():
    """MPC 12/4/10: base vectors, the merged program's tables and eight work vectors fit the 160 KiB LDS"""
    from cvxpygen_amd import solve_program as spm
    d = families.mpc(12, 4, 10)
    plan = build_family_plan(d)
    o = plan.osqp_shared or plan.osqp
    Ps, As = o.pruned(d.P, d.A)
    from cvxpygen_amd import refactor_plan as rp
    mg = rp.shared_mode_plan(Ps, As, o).merged
    assert mg is not None
    steps = spm.execution_steps(mg.sol)
    n_regs = codegen.pack_step_registers(mg.sol, steps)[2]
    lds = codegen.shared_register_lds_bytes(d.n_var, d.m, len(steps), mg.sol.n_chunks, mg.sol.n_slots, n_regs)
    assert lds <= codegen.LDS_BYTES

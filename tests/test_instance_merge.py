"""Merged program of shared-matrix mode's generated instance executor (refactor_plan.shared_mode_plan with `merged`): the
handed-over instances of a rho adaptation solve with a factor whose narrow, consecutive levels are merged into groups, the
diagonal block of every group inverted per instance on the device (resident_plan.py).

CPU tier: the plan's algebra against dense linear algebra, the choice between the merged and the plain program, and the
kernel SOURCES on the lock-step emulator against the C oracle (iteration counts and statuses exact)."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from cvxpygen_amd import codegen, families, refactor_plan as rp, resident_plan as rs, solve_program as spm
from cvxpygen_amd.runtime import BatchSolver, build_family_plan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _shared(d):
    plan = build_family_plan(d)
    o = plan.osqp_shared or plan.osqp
    Ps, As = o.pruned(d.P, d.A)
    return plan, o, Ps, As


def _dense_kkt(pl, Ps, As, sigma, rho_inv):
    n, m = pl.n, pl.m
    pr = pl.Pi; pc = np.repeat(np.arange(n), np.diff(pl.Pp))
    Pm = sp.csc_matrix((Ps, (pr, pc)), shape=(n, n)).toarray(); Pm = Pm + np.triu(Pm, 1).T
    Am = sp.csc_matrix((As, pl.Ai, pl.Ap), shape=(m, n)).toarray()
    return np.block([[Pm + sigma * np.eye(n), Am.T], [Am, -np.diag(rho_inv)]])


@pytest.mark.parametrize('fam', ['mpc12', 'mpc6'])
def test_merged_plan_replay_matches_dense_solve(fam):
    """factorisation + block inverses (combined schedule) and the merged substitution program == a dense solve of K(rho),
    at several rho (equality rows 1e3 rho, as the kernel sets them)"""
    d = families.mpc(12, 4, 10) if fam == 'mpc12' else families.mpc(6, 3, 10)
    plan, o, Ps, As = _shared(d)
    pl = rp.shared_mode_plan(Ps, As, o)
    mg = pl.merged
    assert mg is not None and mg.nnzX > 0 and any(a != b for a, b in mg.groups)
    N = pl.n + pl.m
    assert np.array_equal(mg.sol.final_pos, np.arange(N))
    sigma = o.settings['sigma']
    rng = np.random.default_rng(3)
    for rho in (1e-4, 0.1, 3.0, 1e3):
        rho_inv = 1.0 / np.where(np.arange(pl.m) < d.n_eq, 1e3 * rho, rho)
        fac = rs.replay_factor(mg, Ps.data, As.data, sigma, rho_inv)
        K = _dense_kkt(pl, Ps.data, As.data, sigma, rho_inv)
        rhs = rng.standard_normal(N)
        w = np.zeros(mg.sol.n_slots); w[:N] = rhs
        w = spm.execute_ragged(dataclasses.replace(mg.sol, vals=rs.replay_solve_vals(mg, fac)), w)
        xr = np.linalg.solve(K, rhs)
        assert np.abs(w[:N] - xr).max() <= 1e-12 * np.abs(xr).max(), rho


def test_mpc12_merged_program_depth_and_fit():
    """MPC 12/4/10 (the headline family): the merged program halves the dependent phases of a KKT solve and still fits the
    generated executor -- coefficient registers, LDS slices of [M | 1/d | X | 1.0 | 0.0]"""
    plan, o, Ps, As = _shared(families.mpc(12, 4, 10))
    pl = rp.shared_mode_plan(Ps, As, o)
    plain = rp.shared_mode_plan(Ps, As, o, merge=False)
    assert pl.merged is not None and plain.merged is None
    assert pl.sol.fingerprint() == plain.sol.fingerprint()                 # the streaming executor's tables stay the plain plan's
    steps = spm.execution_steps(pl.merged.sol)
    assert pl.merged.sol.n_phases <= 33 and 2 * pl.merged.sol.n_phases < plain.sol.n_phases
    assert len(steps) < len(spm.execution_steps(plain.sol))
    assert codegen.pack_step_registers(pl.merged.sol, steps)[2] <= codegen.GENI_MAX_REGS
    assert codegen.instance_program_fits(pl)


def test_program_that_does_not_fit_keeps_the_plain_plan(monkeypatch):
    """a merged program over the register budget (or no merging at all) leaves today's plan"""
    plan, o, Ps, As = _shared(families.mpc(12, 4, 10))
    plain = rp.shared_mode_plan(Ps, As, o, merge=False)
    monkeypatch.setattr(rs, 'INSTANCE_MAX_GROUP_ROWS', 64)                 # 8 groups, 92 coefficient registers
    big = rp._merged_variant(plain, Ps, As, o)
    assert big is not None and not codegen.instance_program_fits(big)
    pl = rp.shared_mode_plan(Ps, As, o)
    assert pl.merged is None and pl.sol.fingerprint() == plain.sol.fingerprint()
    monkeypatch.setattr(rs, 'INSTANCE_MAX_GROUP_ROWS', 0)
    assert rp.shared_mode_plan(Ps, As, o).merged is None


def test_merged_instance_executor_on_the_emulator(oracle_lib, tmp_path):
    """the family library's generated instance executor runs the merged program (the header says so, the runtime hands it
    over, the library takes it) and gives the oracle's iteration counts and statuses through several rho adaptations; the
    streaming executor of the same handle keeps the plain tables"""
    import ctypes as C
    from sim import build_sim
    from test_sim_kernel import _assert_parity, _oracle_flat, _theta
    d = families.mpc(6, 3, 10)
    plan = build_family_plan(d)
    lib = build_sim.build_family(plan, str(tmp_path), 'mpc6')
    hdr = open(os.path.join(str(tmp_path), 'cpg_instance_mpc6.h')).read()
    assert '#define CPG_GENI_NNZX ' in hdr and '#define CPG_GENI_FAC_ONE ' in hdr
    vals = -2 + 4 * np.random.default_rng(4).random((4, 6))
    for executor in ('generated', 'stream'):
        bs = BatchSolver(d, lib_path=lib, plan=plan)
        bs.set_launch(waves_per_block=2)
        bs.set_updated(['x_init'])
        assert bs._hybrid
        if executor == 'stream':
            bs.lib.check(bs.lib.L.cpg_hip_set_program_placement(bs.h_rs, 0), 'placement')
        for stg in ({}, dict(eps_abs=1e-7, eps_rel=1e-7), dict(max_iter=60)):
            r = bs.solve({'x_init': vals}, updated_params=['x_init'], **stg)
            assert bs._rplan_s is not None and bs._rplan_s.merged is not None
            v = C.c_double(-1)
            bs.lib.check(bs.lib.L.cpg_hip_get_setting(bs.h_rs, b'generated_instance_executor', C.byref(v)), 'get')
            assert v.value == (1.0 if executor == 'generated' else 0.0)
            o, prim, dual = _oracle_flat(oracle_lib, d, _theta(d, 'x_init', vals), ['x_init'], **stg)
            _assert_parity(r, o, prim, dual)
            if 'eps_abs' in stg:
                assert o['iter'].max() > 100          # more than one adaptation point was passed
        bs.close()


def test_plain_library_keeps_its_generated_executor(oracle_lib, tmp_path, monkeypatch):
    """a library generated without the merge (its header carries the plain program) still runs the generated executor with
    the plain plan: the runtime matches the header's fingerprint against both programs"""
    import ctypes as C
    from sim import build_sim
    from test_sim_kernel import _assert_parity, _oracle_flat, _theta
    d = families.mpc(6, 3, 10)
    plan = build_family_plan(d)
    monkeypatch.setattr(rs, 'INSTANCE_MAX_GROUP_ROWS', 0)
    lib = build_sim.build_family(plan, str(tmp_path), 'mpc6')
    assert '#define CPG_GENI_NNZX ' not in open(os.path.join(str(tmp_path), 'cpg_instance_mpc6.h')).read()
    monkeypatch.undo()
    vals = -2 + 4 * np.random.default_rng(5).random((3, 6))
    bs = BatchSolver(d, lib_path=lib, plan=plan)
    bs.set_launch(waves_per_block=2)
    bs.set_updated(['x_init'])
    stg = dict(eps_abs=1e-7, eps_rel=1e-7)
    r = bs.solve({'x_init': vals}, updated_params=['x_init'], **stg)
    assert bs._rplan_s.merged is None
    v = C.c_double(-1)
    bs.lib.check(bs.lib.L.cpg_hip_get_setting(bs.h_rs, b'generated_instance_executor', C.byref(v)), 'get')
    assert v.value == 1.0
    o, prim, dual = _oracle_flat(oracle_lib, d, _theta(d, 'x_init', vals), ['x_init'], **stg)
    _assert_parity(r, o, prim, dual)
    bs.close()

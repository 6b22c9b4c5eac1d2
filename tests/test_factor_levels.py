"""The instance kernel's generated factorisation emitted level by level (codegen.emit_factor_program(by_level=True), the
instance header only): all operand gathers of a level first, then every chunk's arithmetic in the order and form of the
chunk-by-chunk text, then the level's stores; idle lanes store to a dummy position behind the 0.0 of the factor slice
instead of branching around the store; the reciprocal only in chunks that store a pivot.  Every destination is computed
by the same operations in the same order, so the factor and the coefficients extracted from it
(csrc/cpg_osqp_refactor.h load_instance_coefficients) are the chunk-by-chunk form's bit for bit.

CPU tier: the lock-step emulator on MPC 6/3/10 -- the smallest family with a merged schedule: 57 chunks in 44 levels, among
them levels 2, 3 and 5 chunks wide, chunks of every kind -- built twice, by level and with the option off; toy_box with a
row in another class (the set-up factorisation site); properties of the emitted text for MPC 12/4/10 and MPC 6/3/10.
GPU tier: the MPC 6/3/10 library __graft_entry__.build() compiles for gfx950."""
import ctypes as C
import hashlib
import os
import re
import sys
import types

import numpy as np
import pytest

from cvxpygen_amd import codegen, families, refactor_plan
from cvxpygen_amd.runtime import BatchSolver, build_family_plan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# sha256 of emit_factor_program's text at the commit in front of the by-level form (taken there, from its own output):
# the instance header's factorisation of MPC 6/3/10, and the resident header's of portfolio(100, 10)
PARENT_SHA_MPC6 = '51ddbd5ac6f2d39df2da4c9d3fcc50dea072107f3b01f7b0e20d336c7d2761cc'
PARENT_SHA_PORTFOLIO_RESIDENT = '637f3a815ee357cddd9d4cca46179d20d164ae06da76739000f6d350f769ce1e'


def _shared_plan(d, plan=None):
    plan = plan or build_family_plan(d)
    o = plan.osqp_shared or plan.osqp
    Ps, As = o.pruned(d.P, d.A)
    return refactor_plan.shared_mode_plan(Ps, As, o)


def _factor_text(rpl, by_level):
    mg = rpl.merged
    ns = types.SimpleNamespace(ctab=mg.f_ctab, tlen=mg.f_len, task=mg.f_task)
    return codegen.emit_factor_program(ns, rpl.nnzL, rpl.n + rpl.m, zero=mg.fac_len - 1, one=mg.one_pos,
                                       inverse_from=mg.base.fac.n_chunks, by_level=by_level)


@pytest.fixture(scope='module')
def mpc6():
    d = families.mpc(6, 3, 10)
    return d, build_family_plan(d)


@pytest.fixture(scope='module')
def two_builds(tmp_path_factory, mpc6):
    """emulator libraries of MPC 6/3/10: {True: by level, False: the option off (CPG_FACTOR_BY_LEVEL=0)} -> (library, header)"""
    from sim import build_sim
    d, plan = mpc6
    out, keep = {}, codegen.FACTOR_BY_LEVEL
    try:
        for by_level in (True, False):
            codegen.FACTOR_BY_LEVEL = by_level
            dir_ = str(tmp_path_factory.mktemp('levels' if by_level else 'chunks'))
            lib = build_sim.build_family(plan, dir_, 'mpc6')
            out[by_level] = (lib, open(os.path.join(dir_, 'cpg_instance_mpc6.h')).read())
    finally:
        codegen.FACTOR_BY_LEVEL = keep
    assert '#define CPG_GENI_FAC_BY_LEVEL 1' in out[True][1] and 'CPG_GENI_FAC_BY_LEVEL' not in out[False][1]
    return out


@pytest.fixture(scope='module')
def reference(oracle_lib, mpc6):
    """the oracle on the 48-instance sample of tests/test_single_kernel_step.py (that file shows from the oracle alone that
    the sample holds instances that terminate early, that adapt rho at 50 and that stay in the band), computed once; and
    the number of instances that adapt at 50, told by the oracle as there"""
    from test_single_kernel_step import _sample
    from test_sim_kernel import _oracle_flat, _theta
    d, _ = mpc6
    v = _sample()
    th = _theta(d, 'x_init', v)
    o, prim, dual = _oracle_flat(oracle_lib, d, th, ['x_init'])
    o_ad = oracle_lib.cpg_solve_batch(d, th, ['x_init'], max_iter=74)
    o_fx = oracle_lib.cpg_solve_batch(d, th, ['x_init'], max_iter=74, adaptive_rho=0)
    adapts = (o['iter'] > 50) & ~((o_ad['sol_x'] == o_fx['sol_x']).all(axis=1) & (o_ad['sol_y'] == o_fx['sol_y']).all(axis=1))
    assert adapts.any() and (o['iter'] < 50).any() and o['iter'].max() < 100
    return v, o, prim, dual, int(adapts.sum())


def _solve(d, plan, lib, placement, v, waves=2):
    bs = BatchSolver(d, lib_path=lib, plan=plan)
    if waves:
        bs.set_launch(waves_per_block=waves)
    bs.set_program_placement(placement)
    r = bs.solve({'x_init': v}, updated_params=['x_init'])
    s = C.c_double(-1)
    bs.lib.check(bs.lib.L.cpg_hip_get_setting(bs.h_shared, b'single_kernel_step', C.byref(s)), 'get')
    phase = bs.last_phase_ms()
    bs.close()
    return r, phase, s.value


# ------------------------------------------------------------------------------------------ CPU tier: the emulator
def test_two_builds_agree_bit_for_bit(mpc6, two_builds, reference):
    """placement 5 (the single-kernel step: instances that adapt refactor in the loop): iteration counts and statuses
    identical, primal and dual results and objective values BIT-identical between the by-level build and the build with
    the option off; both match the oracle; both count the adapting instances"""
    from test_sim_kernel import _assert_parity
    d, plan = mpc6
    v, o, prim, dual, n_adapt = reference
    res = {}
    for by_level in (True, False):
        r, phase, single = _solve(d, plan, two_builds[by_level][0], 5, v)
        assert single == 1.0          # (the C++ fit arithmetic agrees with codegen.instance_program_fits on the grown slice)
        _assert_parity(r, o, prim, dual)
        assert phase[2] == n_adapt
        res[by_level] = r
    a, b = res[True], res[False]
    assert a.iter.tolist() == b.iter.tolist() and a.status.tolist() == b.status.tolist()
    assert np.array_equal(a.prim_flat, b.prim_flat) and np.array_equal(a.dual_flat, b.dual_flat)
    assert np.array_equal(a.obj_val, b.obj_val)


def _device_registers(d, plan, lib, nregs, waves=2):
    """debug stage 21: (the family's table as the fast path loads it, the coefficient registers of the device's own
    factorisation -- the table installed under a wrong rho stamp, so every instance factors)"""
    from test_single_kernel_step import _install
    rho = float(plan.osqp.settings['rho'])
    bs = BatchSolver(d, lib_path=lib, plan=plan)
    if waves:
        bs.set_launch(waves_per_block=waves)
    bs.set_program_placement(-1)
    bs.set_updated(['x_init'])
    v = np.tile(-2 + 4 * np.random.default_rng(3).random((1, 6)), (nregs, 1))
    bs._settings_kwargs = dict(debug_stage=21)
    bs._apply_settings_to(bs.h_rs)
    _install(bs, plan, d, rho)                    # replay_factor / replay_solve_vals on the host
    tab = bs._solve_on(bs.h_rs, v, nregs, None, False)[0][:, :64].copy()
    _install(bs, plan, d, 2.0 * rho)              # (stamp of another rho: the kernel factors)
    dev = bs._solve_on(bs.h_rs, v, nregs, None, False)[0][:, :64].copy()
    bs.close()
    return tab, dev


def _assert_registers_match_replay(tab, dev):
    # the tolerance of tests/test_single_kernel_step.py::test_table_equals_the_device_factorisation: 1e-12 relative, of the
    # table's largest entry and entry by entry (both sides run the same dot-product schedule in double precision)
    assert np.isfinite(tab).all() and np.isfinite(dev).all()
    assert (tab != 0.0).sum() > 64 and ((tab == 0.0) == (dev == 0.0)).all()
    print('host replay vs device factorisation: max abs', np.abs(tab - dev).max(), 'max entry', np.abs(tab).max())
    assert np.abs(tab - dev).max() <= 1e-12 * np.abs(tab).max()
    assert (np.abs(tab - dev) <= 1e-12 * np.abs(tab)).all()


def test_device_factorisation_registers(mpc6, two_builds):
    """the coefficient registers the device's own factorisation leaves: bit-identical between the two builds, and the host
    replay's within 1e-12"""
    d, plan = mpc6
    nregs = int(re.search(r'#define CPG_GENI_NREGS (\d+)', two_builds[True][1]).group(1))
    out = {bl: _device_registers(d, plan, two_builds[bl][0], nregs) for bl in (True, False)}
    assert np.array_equal(out[True][1], out[False][1])
    assert np.array_equal(out[True][0], out[False][0])
    _assert_registers_match_replay(*out[True])


def test_row_in_another_class_factors_at_set_up(oracle_lib, tmp_path):
    """toy_box with an upper bound above the infinity threshold (the recipe of tests/test_single_kernel_step.py::
    test_row_in_another_class_factors_on_the_device): such an instance does not start from the family's table, it runs the
    by-level factorisation at the SET-UP site -- parity with the oracle, next to instances that use the table"""
    from sim import build_sim
    d = families.toy_box()
    plan = build_family_plan(d)
    lib = build_sim.build_family(plan, str(tmp_path), 'toy_box')
    hdr = open(os.path.join(str(tmp_path), 'cpg_instance_toy_box.h')).read()
    assert '#define CPG_GENI_NNZX ' in hdr and '#define CPG_GENI_FAC_BY_LEVEL 1' in hdr
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
    bs = BatchSolver(d, lib_path=lib, plan=plan)
    bs.set_launch(waves_per_block=2)
    bs.set_program_placement(-1)
    r = bs.solve(updated_params=upd, theta_var=tv)
    s = C.c_double(-1)
    bs.lib.check(bs.lib.L.cpg_hip_get_setting(bs.h_shared, b'single_kernel_step', C.byref(s)), 'get')
    bs.close()
    assert s.value == 1.0
    assert r.iter.tolist() == o['iter'].tolist() and r.status.tolist() == o['status'].tolist()
    ok = np.isin(o['status'], (1, 2, 7))
    assert ok[[1, 3]].all()
    sol = np.concatenate([o['sol_x'][:, v.indices] for v in d.variables], axis=1)
    assert np.abs(r.prim_flat[ok] - sol[ok]).max() <= 1e-9 * max(1.0, np.abs(sol[ok]).max())
    assert np.abs(r.obj_val[ok] - o['obj_val'][ok]).max() <= 1e-9 * max(1.0, np.abs(o['obj_val'][ok]).max())


# ------------------------------------------------------------------------------------------ the emitted text
@pytest.mark.parametrize('fam', ['mpc12', 'mpc6'])
def test_generator_properties(fam):
    d = families.mpc(12, 4, 10) if fam == 'mpc12' else families.mpc(6, 3, 10)
    rpl = _shared_plan(d)
    mg = rpl.merged
    assert mg is not None
    text = _factor_text(rpl, True)
    body = text[text.index('CPG_DEV void numeric_ldl_gen'):]
    ct = np.asarray(mg.f_ctab, dtype=np.int64).reshape(-1, 4)
    # the levels of the schedule, counted here: chunks up to and including one whose bit 0 of column 1 is set
    ends = np.nonzero(ct[:, 1] & 1)[0]
    n_levels = len(ends) + (0 if ends[-1] == len(ct) - 1 else 1)
    parts = re.split(r'^    // level \d+:.*$', body, flags=re.M)
    assert len(parts) == n_levels + 1
    if fam == 'mpc6':
        widths = np.diff(np.concatenate([[-1], ends]))
        assert len(ct) == 57 and n_levels == 44 and {2, 3, 5} <= set(widths.tolist())
    n_gather = n_store = 0
    for lvl in parts[1:]:
        lines = lvl.splitlines()
        gathers = [i for i, l in enumerate(lines) if re.search(r'= w\[', l)]
        stores = [i for i, l in enumerate(lines) if re.match(r'\s+w\[[^\]]*\] = ', l)]
        assert stores, 'a level without a store'
        # within every level, no store precedes the level's last gather
        assert not gathers or min(stores) > max(gathers)
        order = [i for i, l in enumerate(lines) if 'cpgw::lds_order();' in l]
        assert len(order) == 1 and order[0] > max(stores)         # one ordering point per level, behind its stores
        n_gather += len(gathers)
        n_store += len(stores)
    assert n_store == len(ct) and n_gather == int(ct[:, 0].sum())       # one store per chunk, one gather line per step
    # no test of the destination remains, and no branch
    assert '!= 0xFFFFu' not in body and '== 0xFFFFu' not in body and 'if (' not in body
    # the reciprocal only where a pivot is stored: chunks of the LDL' part with a destination among the N reciprocal pivots
    # [nnzL, nnzL + N), from the schedule's task table
    N = rpl.n + rpl.m
    task = np.asarray(mg.f_task, dtype=np.int64).reshape(len(ct), -1)
    n_ldl = mg.base.fac.n_chunks
    with_pivot = 0
    for c in range(n_ldl):
        t = task[c][task[c] != 0xFFFFFFFF] & 0x7FFFFFFF
        with_pivot += bool(((t >= rpl.nnzL) & (t < rpl.nnzL + N)).any())
    assert with_pivot > 0 and text.count('1.0 /') == with_pivot
    # the fit arithmetic holds on the grown slice
    assert codegen.FACTOR_BY_LEVEL and codegen.instance_program_fits(rpl)
    assert mg.fac_len + codegen.FACTOR_DUMMY_DOUBLES < 0xFFFF


def test_option_off_reproduces_the_parent_text():
    """with the option off, emit_factor_program gives the text of the commit in front of the by-level form, byte for byte:
    checked against a sha256 taken at that commit from its own output, for the instance header's factorisation of MPC
    6/3/10; and the resident header's factor text (preloaded form, untouched by the option) of portfolio(100, 10)"""
    rpl = _shared_plan(families.mpc(6, 3, 10))
    assert hashlib.sha256(_factor_text(rpl, False).encode()).hexdigest() == PARENT_SHA_MPC6
    assert _factor_text(rpl, True) != _factor_text(rpl, False)
    from cvxpygen_amd import resident_plan as rs
    d = families.portfolio(100, 10)
    plan = build_family_plan(d)
    rp = rs.build_resident_plan(d.P, d.A, plan.osqp)
    b = rp.base
    t = codegen.emit_factor_program(types.SimpleNamespace(ctab=rp.f_ctab, tlen=rp.f_len), b.nnzL, b.n + b.m, prefix='GENR',
                                    preloaded=True, func='resident_factor_gen', zero=rp.fac_len - 1)
    assert hashlib.sha256(t.encode()).hexdigest() == PARENT_SHA_PORTFOLIO_RESIDENT


# ------------------------------------------------------------------------------------------ GPU tier
@pytest.fixture(scope='module')
def gpu_lib(mpc6, tmp_path_factory):
    """the MPC 6/3/10 family library compiled with hipcc (what __graft_entry__.build() leaves: a no-op when it matches the
    plan and the sources)"""
    d, plan = mpc6
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cvxpygen_amd', 'generated', 'mpc6')
    if os.path.exists(os.path.join(root, 'libcpg_mpc6.so')) and os.path.exists(os.path.join(root, 'cpg_instance_mpc6.h')):
        out = root
    else:
        out = str(tmp_path_factory.mktemp('gpu_levels'))
    lib = codegen.build_family_library(plan, out, 'mpc6')
    hdr = open(os.path.join(out, 'cpg_instance_mpc6.h')).read()
    assert '#define CPG_GENI_FAC_BY_LEVEL 1' in hdr
    return lib, int(re.search(r'#define CPG_GENI_NREGS (\d+)', hdr).group(1))


@pytest.mark.gpu
def test_sample_on_the_gpu(mpc6, gpu_lib, reference):
    """placements 5 (single kernel: in-loop refactorisation) and 1 (two kernels: the instance kernel factors at its start):
    iteration counts and statuses equal between them and to the oracle, primal and dual results within the 1e-6 of the GPU
    parity tests, the same hand-over count"""
    from test_sim_kernel import _assert_parity
    d, plan = mpc6
    v, o, prim, dual, n_adapt = reference
    res = {}
    for placement in (5, 1):
        r, phase, single = _solve(d, plan, gpu_lib[0], placement, v, waves=None)
        assert single == (1.0 if placement == 5 else 0.0)
        print('placement', placement, 'max abs prim', np.abs(r.prim_flat - prim).max(), 'dual', np.abs(r.dual_flat - dual).max())
        _assert_parity(r, o, prim, dual, tol=1e-6)
        res[placement] = (r, phase)
    assert res[5][0].iter.tolist() == res[1][0].iter.tolist() and res[5][0].status.tolist() == res[1][0].status.tolist()
    assert res[5][1][2] == res[1][1][2] == n_adapt


@pytest.mark.gpu
def test_device_factorisation_registers_on_the_gpu(mpc6, gpu_lib):
    d, plan = mpc6
    _assert_registers_match_replay(*_device_registers(d, plan, gpu_lib[0], gpu_lib[1], waves=None))

"""The instance kernel's coefficient extraction in two passes (csrc/cpg_osqp_refactor.h gather_instance_coefficients, headers
with CPG_GENI_COEF_TWO_PASS): the L entries behind kind-2 coefficients are scaled in place, M[e] = -(M[e] * Dinv[col_e]), each
once, from a host-built list; then a coefficient register is one LDS read at a host-built byte offset into the factor slice
[M | 1/d | X | 1.0 | 0.0 | dummy].  The product and the negation are load_instance_coefficients', so the registers -- and
everything computed from them -- are the register-by-register form's bit for bit.

CPU tier: the lock-step emulator on MPC 6/3/10 built twice (codegen.COEFFICIENT_TWO_PASS on and off); the two tables read back
through cpg_hip_get_coefficient_tables for MPC 12/4/10 and MPC 6/3/10 against a numpy restatement from the plan; toy_box with a
row in another class (the set-up site); a library without a merged program (the old function); the header text with the
option off.  GPU tier: the MPC 6/3/10 library __graft_entry__.build() compiles for gfx950."""
import ctypes as C
import hashlib
import os
import re
import sys

import numpy as np
import pytest

from cvxpygen_amd import codegen, families
from cvxpygen_amd import resident_plan as rs
from cvxpygen_amd.runtime import BatchSolver, build_family_plan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_factor_levels import (_assert_registers_match_replay, _device_registers, _shared_plan, _solve,   # noqa: E402
                                mpc6, reference)                                                           # noqa: E402,F401

# sha256 of cpg_instance_mpc6.h as codegen.instance_header writes it at the commit in front of the two-pass extraction (taken
# there, from its own output)
PARENT_SHA_INSTANCE_HEADER_MPC6 = 'f5e4463fbb9d7fa7b83c4e9f79870a3695b16ca0d12f6073db4d4c2393d13aaa'


def _define(hdr, name):
    m = re.search(r'^#define %s (\d+)u?$' % name, hdr, re.M)
    return int(m.group(1)) if m else None


@pytest.fixture(scope='module')
def two_builds(tmp_path_factory, mpc6):
    """emulator libraries of MPC 6/3/10: {True: two passes, False: the option off} -> (library, instance header)"""
    from sim import build_sim
    d, plan = mpc6
    out, keep = {}, codegen.COEFFICIENT_TWO_PASS
    try:
        for on in (True, False):
            codegen.COEFFICIENT_TWO_PASS = on
            dir_ = str(tmp_path_factory.mktemp('two_pass' if on else 'by_register'))
            lib = build_sim.build_family(plan, dir_, 'mpc6')
            out[on] = (lib, open(os.path.join(dir_, 'cpg_instance_mpc6.h')).read())
    finally:
        codegen.COEFFICIENT_TWO_PASS = keep
    assert '#define CPG_GENI_COEF_TWO_PASS 1' in out[True][1] and 'COEF_TWO_PASS' not in out[False][1]
    assert '#define CPG_GENI_FAC_BY_LEVEL 1' in out[False][1]
    return out


# ------------------------------------------------------------------------------------------ CPU tier: the emulator
def test_two_builds_agree_bit_for_bit(mpc6, two_builds, reference):
    """placement 5 (instances that adapt refactor in the loop): iteration counts and statuses identical, primal and dual results
    and objective values BIT-identical between the two builds; both match the oracle; both count the adapting instances"""
    from test_sim_kernel import _assert_parity
    d, plan = mpc6
    v, o, prim, dual, n_adapt = reference
    res = {}
    for on in (True, False):
        r, phase, single = _solve(d, plan, two_builds[on][0], 5, v)
        assert single == 1.0
        _assert_parity(r, o, prim, dual)
        assert phase[2] == n_adapt and n_adapt > 0
        res[on] = r
    a, b = res[True], res[False]
    assert a.iter.tolist() == b.iter.tolist() and a.status.tolist() == b.status.tolist()
    assert np.array_equal(a.prim_flat, b.prim_flat) and np.array_equal(a.dual_flat, b.dual_flat)
    assert np.array_equal(a.obj_val, b.obj_val)


def test_device_factorisation_registers(mpc6, two_builds):
    """debug stage 21, the table installed under a wrong rho stamp so that every instance factors: all NREGS x 64 coefficient
    registers bit-identical between the two builds, and within 1e-12 of the host replay"""
    d, plan = mpc6
    nregs = _define(two_builds[True][1], 'CPG_GENI_NREGS')
    out = {on: _device_registers(d, plan, two_builds[on][0], nregs) for on in (True, False)}
    assert out[True][1].shape == (nregs, 64)
    assert np.array_equal(out[True][1], out[False][1])
    assert np.array_equal(out[True][0], out[False][0])
    _assert_registers_match_replay(*out[True])


def _expected_sources(rpl, hdr):
    """numpy restatement from the plan and the header's step list {first entry, lanes, register, lane shift}: per (register,
    lane) the position in the slice [M | 1/d | X | 1.0 | 0.0] its coefficient comes from today -- (kind, idx) of the program entry:
    2 -> M[idx] (to be scaled by the reciprocal pivot of column Lcol[idx]), 3 -> 1/d[idx], 4 -> X[idx], 1 -> the 1.0, 0 and
    untaken lanes -> the 0.0 -- and the set of M entries behind kind-2 coefficients"""
    mg = rpl.merged
    N, nnzL = rpl.n + rpl.m, rpl.nnzL
    steps = [[int(x) for x in t.split(',')] for t in re.findall(r'\{(\d+, \d+, \d+, \d+)\}', re.search(r'#define CPG_GENI_STEPS \{(.*)\}', hdr).group(1))]
    nregs, zero, one = _define(hdr, 'CPG_GENI_NREGS'), _define(hdr, 'CPG_GENI_FAC_ZERO'), _define(hdr, 'CPG_GENI_FAC_ONE')
    assert one == nnzL + N + mg.nnzX and zero == one + 1 == mg.fac_len - 1
    pos = np.full((nregs, 64), zero, dtype=np.int64)
    taken = np.zeros((nregs, 64), dtype=bool)
    kind2 = set()
    for e, cnt, reg, sh in steps:
        for l in range(cnt):
            k, i = int(mg.sol_kind[e + l]), int(mg.sol_idx[e + l])
            assert not taken[reg, l + sh]
            taken[reg, l + sh] = True
            if k == 2:
                assert 0 <= i < nnzL
                kind2.add(i)
            pos[reg, l + sh] = {0: zero, 1: one, 2: i, 3: nnzL + i, 4: nnzL + N + i}[k]
    return pos, taken, kind2, zero


@pytest.mark.parametrize('fam', ['mpc12', 'mpc6'])
def test_table_properties(fam, tmp_path, mpc6):
    from sim import build_sim
    if fam == 'mpc6':
        d, plan = mpc6
    else:
        d = families.mpc(12, 4, 10)
        plan = build_family_plan(d)
    lib = build_sim.build_family(plan, str(tmp_path), fam)
    hdr = open(os.path.join(str(tmp_path), f'cpg_instance_{fam}.h')).read()
    rounds, nregs = _define(hdr, 'CPG_GENI_COEF_SCALE_ROUNDS'), _define(hdr, 'CPG_GENI_NREGS')
    assert '#define CPG_GENI_COEF_TWO_PASS 1' in hdr and rounds > 0
    rpl = _shared_plan(d, plan)
    pos_x, taken, kind2, zero = _expected_sources(rpl, hdr)
    bs = BatchSolver(d, lib_path=lib, plan=plan)
    bs.set_updated(['x_init'])
    scale = np.zeros(64 * rounds, dtype=np.uint32)
    off = np.zeros(64 * nregs, dtype=np.uint16)
    n_ent = C.c_int32(-1)
    bs.lib.check(bs.lib.L.cpg_hip_get_coefficient_tables(bs.h_rs, scale.ctypes.data_as(C.POINTER(C.c_uint32)), scale.size,
                                                        off.ctypes.data_as(C.POINTER(C.c_uint16)), off.size, C.byref(n_ent)),
                 'get_coefficient_tables')
    bs.close()
    off = off.astype(np.int64).reshape(nregs, 64)
    slice_bytes = 8 * (zero + 1 + codegen.FACTOR_DUMMY_DOUBLES)
    assert slice_bytes <= 0xFFFF
    # every offset a multiple of 8 inside the slice; decoded, today's source of every (register, lane); untaken lanes the 0.0
    assert (off % 8 == 0).all() and (off >= 0).all() and (off < slice_bytes).all()
    assert np.array_equal(off // 8, pos_x)
    assert (~taken).any() and (off[~taken] == 8 * zero).all()
    # the scale list: every kind-2 M entry exactly once and nothing else (no pivot, no X entry: positions below nnzL), each
    # with the position of its column's reciprocal pivot; behind it the words of idle lanes (the dummy double, the 0.0)
    n_ent = n_ent.value
    assert n_ent == len(kind2) and rounds == -(-n_ent // 64)
    ent, piv = (scale & 0xFFFF).astype(np.int64), (scale >> 16).astype(np.int64)
    assert len(set(ent[:n_ent].tolist())) == n_ent and set(ent[:n_ent].tolist()) == kind2
    assert (ent[:n_ent] < rpl.nnzL).all()
    assert np.array_equal(piv[:n_ent], rpl.nnzL + np.asarray(rpl.Lcol, dtype=np.int64)[ent[:n_ent]])
    assert (piv[:n_ent] < rpl.nnzL + rpl.n + rpl.m).all()
    assert (ent[n_ent:] == zero + 1).all() and (piv[n_ent:] == zero).all()


def test_row_in_another_class_factors_at_set_up(oracle_lib, tmp_path):
    """toy_box with an upper bound above the infinity threshold (the recipe of tests/test_factor_levels.py::
    test_row_in_another_class_factors_at_set_up): such an instance does not start from the family's table, it factors -- and
    extracts its coefficients in two passes -- at the SET-UP site; parity with the oracle, next to instances that use the table"""
    from sim import build_sim
    d = families.toy_box()
    plan = build_family_plan(d)
    lib = build_sim.build_family(plan, str(tmp_path), 'toy_box')
    hdr = open(os.path.join(str(tmp_path), 'cpg_instance_toy_box.h')).read()
    assert '#define CPG_GENI_NNZX ' in hdr and '#define CPG_GENI_COEF_TWO_PASS 1' in hdr
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


def test_library_without_a_merged_program_keeps_the_old_function(oracle_lib, tmp_path, monkeypatch, mpc6):
    """a library generated with INSTANCE_MAX_GROUP_ROWS = 0 (plain program, factor [M | 1/d | 0.0]): no two-pass switch in its
    header, the getter says so, and it solves in parity through several rho adaptations"""
    from sim import build_sim
    from test_sim_kernel import _assert_parity, _oracle_flat, _theta
    d, plan = mpc6
    monkeypatch.setattr(rs, 'INSTANCE_MAX_GROUP_ROWS', 0)
    lib = build_sim.build_family(plan, str(tmp_path), 'mpc6')
    hdr = open(os.path.join(str(tmp_path), 'cpg_instance_mpc6.h')).read()
    assert '#define CPG_GENI_NNZX ' not in hdr and 'COEF_TWO_PASS' not in hdr and '#define CPG_GENI_FAC_NSTEPS ' in hdr
    monkeypatch.undo()
    vals = -2 + 4 * np.random.default_rng(5).random((3, 6))
    bs = BatchSolver(d, lib_path=lib, plan=plan)
    bs.set_launch(waves_per_block=2)
    bs.set_updated(['x_init'])
    stg = dict(eps_abs=1e-7, eps_rel=1e-7)
    r = bs.solve({'x_init': vals}, updated_params=['x_init'], **stg)
    v = C.c_double(-1)
    bs.lib.check(bs.lib.L.cpg_hip_get_setting(bs.h_rs, b'generated_instance_executor', C.byref(v)), 'get')
    assert v.value == 1.0
    buf32, buf16, n_ent = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint16), C.c_int32(0)
    rc = bs.lib.L.cpg_hip_get_coefficient_tables(bs.h_rs, buf32.ctypes.data_as(C.POINTER(C.c_uint32)), 64,
                                                 buf16.ctypes.data_as(C.POINTER(C.c_uint16)), 64, C.byref(n_ent))
    assert rc != 0
    o, prim, dual = _oracle_flat(oracle_lib, d, _theta(d, 'x_init', vals), ['x_init'], **stg)
    assert o['iter'].max() > 100          # more than one adaptation point was passed
    _assert_parity(r, o, prim, dual)
    bs.close()


def test_option_off_reproduces_the_parent_header(tmp_path, mpc6, monkeypatch):
    """with the option off, codegen.instance_header writes the text of the commit in front of this form, byte for byte
    (sha256 taken at that commit from its own output, MPC 6/3/10); with it on, that text and the switch behind it"""
    d, plan = mpc6
    (tmp_path / 'off').mkdir()
    (tmp_path / 'on').mkdir()
    monkeypatch.setattr(codegen, 'COEFFICIENT_TWO_PASS', False)
    off = open(codegen.instance_header(plan, str(tmp_path / 'off'), 'mpc6')).read()
    assert hashlib.sha256(off.encode()).hexdigest() == PARENT_SHA_INSTANCE_HEADER_MPC6
    monkeypatch.setattr(codegen, 'COEFFICIENT_TWO_PASS', True)
    on = open(codegen.instance_header(plan, str(tmp_path / 'on'), 'mpc6')).read()
    assert on.startswith(off) and on != off
    extra = on[len(off):].splitlines()
    assert extra[0] == '#define CPG_GENI_COEF_TWO_PASS 1' and re.fullmatch(r'#define CPG_GENI_COEF_SCALE_ROUNDS \d+', extra[1])
    assert all(re.fullmatch(r'#define CPG_COEF_(SCALE|OFFSET)_BATCH \d+', l) for l in extra[2:])


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
        out = str(tmp_path_factory.mktemp('gpu_two_pass'))
    lib = codegen.build_family_library(plan, out, 'mpc6')
    hdr = open(os.path.join(out, 'cpg_instance_mpc6.h')).read()
    assert '#define CPG_GENI_COEF_TWO_PASS 1' in hdr
    return lib, _define(hdr, 'CPG_GENI_NREGS')


@pytest.mark.gpu
def test_wavefronts_solve_several_instances_in_sequence(oracle_lib, mpc6, gpu_lib):
    """8 192 instances on the 2 048 resident wavefronts of the single-kernel step, so a wavefront solves about four, one behind
    the other, and the slice and the coefficient registers of one instance are overwritten by the next; x_init at six
    magnitudes, shuffled: instances that start from the family's table and end at the first test next to instances that
    adapt rho and refactor in the loop.  Iteration counts and statuses exact against the oracle, results within the 1e-6 of
    the GPU parity tests; some, and at most the instances that pass iteration 50, refactor in the loop"""
    from test_sim_kernel import _assert_parity, _oracle_flat, _theta
    d, plan = mpc6
    rng = np.random.default_rng(11)
    B = 8192
    mag = rng.choice([0.02, 0.1, 0.3, 1.0, 2.0, 4.0], size=(B, 1))
    v = mag * (-1 + 2 * rng.random((B, 6)))
    th = _theta(d, 'x_init', v)
    o, prim, dual = _oracle_flat(oracle_lib, d, th, ['x_init'])
    early, late = int((o['iter'] < 50).sum()), int((o['iter'] > 50).sum())
    assert early > 1000 and late > 1000
    r, phase, single = _solve(d, plan, gpu_lib[0], 5, v, waves=None)
    assert single == 1.0
    print('instances below / above iteration 50:', early, late, 'refactored in the loop:', phase[2],
          'max abs prim', np.abs(r.prim_flat - prim).max(), 'dual', np.abs(r.dual_flat - dual).max())
    _assert_parity(r, o, prim, dual, tol=1e-6)
    assert 0 < phase[2] <= late


@pytest.mark.gpu
def test_device_factorisation_registers_on_the_gpu(mpc6, gpu_lib):
    d, plan = mpc6
    _assert_registers_match_replay(*_device_registers(d, plan, gpu_lib[0], gpu_lib[1], waves=None))

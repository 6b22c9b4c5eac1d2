"""The lean instance executor (codegen.emit_instance_program(lean=True), the instance kernel's header): output-slot table in
byte offsets, the stages of the segmented reductions as one fused move-and-select (cpgw::seg_sum_first_sel).  Nothing of the
arithmetic changes, so the kernel must give what the table-driven executor and the oracle give -- on MPC 2/1/3, the smallest
MPC family whose merged instance program has a segmented chunk, an accumulating chunk and more than four steps (two table
words per lane), with 130 instances: two full rounds of 64 and a ragged tail on the work counter.  Default settings; then,
because this small family converges at the first test under them, tolerances of 1e-7 (rho adapts, instances refactor in
the loop: the oracle's run must show it) and, at those tolerances, max_iter 1, 25, 26, 50: the iteration right at, in front
of and behind a termination test and the adaptation point.

CPU tier: the lock-step emulator.  GPU tier: the family library __graft_entry__.build() compiles for gfx950."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from cvxpygen_amd import codegen, families
from cvxpygen_amd.runtime import BatchSolver, build_family_plan
from cvxpygen_amd.solve_program import GEN_DUMMY_SLOTS, execution_steps

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NAME = 'mpc2'
B = 130
TIGHT = dict(eps_abs=1e-7, eps_rel=1e-7)
# None: default settings.  At default tolerances every instance of this small family stops at the first test (iteration 25), so
# rho never adapts; at 1e-7 instances pass the adaptation point at 50 and refactor in the loop ('tight': the reference run
# must show that), and max_iter 1, 25, 26, 50 cut the solve at, in front of and behind a test and the adaptation point
MAX_ITERS = (None, 'tight', 1, 25, 26, 50)


def _family():
    return families.mpc(2, 1, 3)


def _values():
    """seeded x_init at six magnitudes: small ones stop at the first test, large ones adapt rho at iteration 50"""
    rng = np.random.default_rng(11)
    v = np.concatenate([s * (-1 + 2 * rng.random((22, 2))) for s in (0.02, 0.1, 0.3, 1.0, 2.0, 4.0)])
    return v[:B]


def _stg(mi):
    return {} if mi is None else (dict(TIGHT) if mi == 'tight' else dict(TIGHT, max_iter=mi))


@pytest.fixture(scope='module')
def fam():
    d = _family()
    return d, build_family_plan(d)


@pytest.fixture(scope='module')
def reference(oracle_lib, fam):
    """the oracle's results per max_iter setting, computed once; and which instances adapt rho at iteration 50, told by the
    oracle alone (cut off at 74, in front of the next test, a solve with adaptation differs from one without exactly then)"""
    from test_sim_kernel import _oracle_flat, _theta
    d, _ = fam
    th = _theta(d, 'x_init', _values())
    ref = {mi: _oracle_flat(oracle_lib, d, th, ['x_init'], **_stg(mi)) for mi in MAX_ITERS}
    o = ref['tight'][0]
    o_ad = oracle_lib.cpg_solve_batch(d, th, ['x_init'], max_iter=74, **TIGHT)
    o_fx = oracle_lib.cpg_solve_batch(d, th, ['x_init'], max_iter=74, adaptive_rho=0, **TIGHT)
    adapts = (o['iter'] > 50) & ~((o_ad['sol_x'] == o_fx['sol_x']).all(axis=1) & (o_ad['sol_y'] == o_fx['sol_y']).all(axis=1))
    assert int(adapts.sum()) > 0 and (o['iter'] <= 50).any()        # (hand-over count of the reference run > 0)
    return ref, int(adapts.sum()) if o['iter'].max() < 100 else None


@pytest.fixture(scope='module')
def sim_family_lib(tmp_path_factory, fam):
    from sim import build_sim
    d, plan = fam
    out = str(tmp_path_factory.mktemp('lean'))
    lib = build_sim.build_family(plan, out, NAME)
    return lib, open(os.path.join(out, f'cpg_instance_{NAME}.h')).read()


def _merged(fam):
    from cvxpygen_amd import refactor_plan
    d, plan = fam
    o = plan.osqp_shared or plan.osqp
    Ps, As = o.pruned(d.P, d.A)
    return refactor_plan.shared_mode_plan(Ps, As, o).merged


def test_family_exercises_the_lean_paths(fam, sim_family_lib):
    """the family's merged program has what the lean executor changes: a segmented chunk, an accumulating chunk, more than
    four steps; and its header is the lean one"""
    mg = _merged(fam)
    assert mg is not None
    kinds = [int(k) for k in mg.sol.ctab[:, 3]]
    assert any(k & 1 for k in kinds) and any(k & 2 for k in kinds) and len(execution_steps(mg.sol)) > 4
    hdr = sim_family_lib[1]
    assert '#define CPG_GENI_LEAN 1' in hdr and '#define CPG_GENI_NNZX ' in hdr
    assert 'cpgw::seg_sum_first_sel<' in hdr and 'CPG_GEN_SLOT_MASK' not in hdr.split('run_program_inst')[1].split('namespace')[0]


def _compare(r, g, o, prim, dual, count=None, phase=None):
    """r: the lean instance kernel's results; g: the table-driven executor's; o, prim, dual: the oracle's"""
    from test_sim_kernel import _assert_parity
    # oracle, as tests/test_single_kernel_step.py: counts and statuses exact, 1e-6 on primal and dual results
    _assert_parity(r, o, prim, dual, tol=1e-6)
    # table-driven executor: counts and statuses exact, results to 1e-9 relative, residuals as _assert_parity takes them
    assert r.iter.tolist() == g.iter.tolist() and r.status.tolist() == g.status.tolist()
    for a, b in ((r.prim_flat, g.prim_flat), (r.dual_flat, g.dual_flat), (r.obj_val, g.obj_val)):
        print('against the table-driven executor: max abs difference', np.abs(a - b).max())
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
    assert np.allclose(r.pri_res, g.pri_res, rtol=1e-6, atol=1e-9) and np.allclose(r.dua_res, g.dua_res, rtol=1e-6, atol=1e-9)
    if count is not None:
        assert phase[2] == count


def _run(d, plan, lib, generic_lib, reference, mi, waves=None):
    ref, count = reference
    o, prim, dual = ref[mi]
    v = _values()
    bs = BatchSolver(d, lib_path=lib, plan=plan)
    if waves:
        bs.set_launch(waves_per_block=waves)
    bs.set_program_placement(5)                 # the single-kernel step: the instance kernel over the whole batch
    r = bs.solve({'x_init': v}, updated_params=['x_init'], **_stg(mi))
    s = C.c_double(-1)
    bs.lib.check(bs.lib.L.cpg_hip_get_setting(bs.h_shared, b'single_kernel_step', C.byref(s)), 'get')
    assert s.value == 1.0
    phase = bs.last_phase_ms()
    bs.close()
    gs = BatchSolver(d, lib_path=generic_lib) if generic_lib else BatchSolver(d)
    if waves:
        gs.set_launch(waves_per_block=waves)
    g = gs.solve({'x_init': v}, updated_params=['x_init'], **_stg(mi))
    gs.close()
    _compare(r, g, o, prim, dual, count if mi == 'tight' else None, phase)
    if mi == 'tight':
        assert phase[2] > 0                     # instances refactored in the loop


@pytest.mark.parametrize('mi', MAX_ITERS)
def test_lean_kernel_on_the_emulator(fam, sim_family_lib, sim_lib, reference, mi):
    d, plan = fam
    _run(d, plan, sim_family_lib[0], sim_lib, reference, mi, waves=2)


def _expected_tables(mg, hdr):
    """numpy restatement of the layout: cols[step / 4][lane][step % 4] = byte offset of the operand the step's entry of that lane
    reads (8 x the slot the plan assigns; lanes without an entry: the zero slot behind the dummy slots); rows[chunk / 4][lane]
    [chunk % 4] = 8 x the slot the lane's row is stored to (lanes without a row: some dummy slot behind the program's own)"""
    sol = mg.sol
    steps = [[int(x) for x in t.split(',')] for t in re.findall(r'\{(\d+, \d+, \d+, \d+)\}', re.search(r'#define CPG_GENI_STEPS \{(.*)\}', hdr).group(1))]
    shift = [int(x) for x in re.search(r'#define CPG_GENI_CHUNK_SHIFT \{(.*)\}', hdr).group(1).split(',')]
    T, nc = len(steps), sol.n_chunks
    assert T == len(execution_steps(sol))
    zero = (sol.n_slots + GEN_DUMMY_SLOTS) * 8
    cols = np.full(((T + 3) // 4, 64, 4), zero, dtype=np.int64)
    for t, (e, cnt, _, sh) in enumerate(steps):
        cols[t // 4, sh:sh + cnt, t % 4] = np.asarray(sol.cols[e:e + cnt], dtype=np.int64)
    rows = np.full(((nc + 3) // 4, 64, 4), -1, dtype=np.int64)
    for c in range(nc):
        slot = (np.asarray(sol.desc[c], dtype=np.int64) & 0xFFFF)
        for l in range(64 - shift[c]):
            if slot[l] != 0xFFFF:
                rows[c // 4, l + shift[c], c % 4] = 8 * slot[l]
    return cols, rows, steps


def _check_tables(fam, lib, hdr):
    d, plan = fam
    mg = _merged(fam)
    cols_x, rows_x, steps = _expected_tables(mg, hdr)
    bs = BatchSolver(d, lib_path=lib, plan=plan)
    bs.set_updated(['x_init'])
    cols = np.zeros(cols_x.size, dtype=np.uint16)
    rows = np.zeros(rows_x.size, dtype=np.uint16)
    rb = C.c_int32(-1)
    p16 = C.POINTER(C.c_uint16)
    bs.lib.check(bs.lib.L.cpg_hip_get_instance_tables(bs.h_rs, cols.ctypes.data_as(p16), cols.size, rows.ctypes.data_as(p16), rows.size,
                                                     C.byref(rb)), 'get_instance_tables')
    bs.close()
    assert rb.value == 1
    cols, rows = cols.astype(np.int64).reshape(cols_x.shape), rows.astype(np.int64).reshape(rows_x.shape)
    # every step: the word a lane reads is 8 x the slot index the plan assigns to that entry's operand
    assert np.array_equal(cols, cols_x)
    sol = mg.sol
    assert (np.asarray(sol.cols[:sol.nnz], dtype=np.int64) % 8 == 0).all() and sol.n_slots * 8 <= int(cols_x.max())
    # every chunk: lanes with a row hold 8 x its slot, the others a dummy slot [n_slots, n_slots + GEN_DUMMY_SLOTS); no flag bits
    real = rows_x >= 0
    real[:, :, :] &= True
    assert np.array_equal(rows[real], rows_x[real])
    pad = ~real
    pad.reshape(-1, 64, 4)[(sol.n_chunks + 3) // 4 - 1, :, sol.n_chunks % 4 or 4:] = False     # (chunks past the last: never read)
    assert (rows[pad] % 8 == 0).all() and (rows[pad] >= 8 * sol.n_slots).all() and (rows[pad] < 8 * (sol.n_slots + GEN_DUMMY_SLOTS)).all()


def test_table_layout_on_the_emulator(fam, sim_family_lib):
    _check_tables(fam, *sim_family_lib)


def _gpu_lib(fam, tmp_path):
    d, plan = fam
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'cvxpygen_amd', 'generated', NAME)
    pre = os.path.join(root, f'libcpg_{NAME}.so')
    if os.path.exists(pre) and os.path.exists(os.path.join(root, f'cpg_instance_{NAME}.h')):
        lib, out = codegen.build_family_library(plan, root, NAME), root       # (a no-op when it matches the plan and the sources)
    else:
        out = str(tmp_path)
        lib = codegen.build_family_library(plan, out, NAME)
    return lib, open(os.path.join(out, f'cpg_instance_{NAME}.h')).read()


@pytest.mark.gpu
@pytest.mark.parametrize('mi', MAX_ITERS)
def test_lean_kernel_on_the_gpu(fam, reference, tmp_path, mi):
    d, plan = fam
    _run(d, plan, _gpu_lib(fam, tmp_path)[0], None, reference, mi)


@pytest.mark.gpu
def test_table_layout_on_the_gpu(fam, tmp_path):
    _check_tables(fam, *_gpu_lib(fam, tmp_path))

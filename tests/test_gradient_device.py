"""Device-resident QP adjoint: cpg_hip_set_gradient_vars / cpg_hip_gradient_batch_device, runtime.DeviceGradBatch and
BatchSolver.gradient_device.  Every case queues the forward solve into a DeviceBatch and the adjoint right behind it --
no host synchronisation in between, only the gradient handle is waited for -- and compares with the host entry point
(cpg_hip_gradient_batch through BatchSolver.gradient) on the same solution, bit for bit, and with the restated adjoint of
oracle/ at the tolerances tests/test_gradient.py uses for the host path (1e-10 relative on nonneg-LS, 1e-8 on the MPC
adjoint).  Families, seeds and input generators are those of tests/test_gradient.py; nonneg-LS (1, 1) is the smaller of
the reference's gradient test shapes (tests/test_diff.py).  The emulator tier runs through the real C-ABI; the GPU tier
repeats the comparisons on the HIP library."""
import ctypes as C

import numpy as np
import pytest

from cvxpygen_amd import families
from cvxpygen_amd.runtime import BatchSolver, DeviceBatch, DeviceGradBatch

CPG_E_BADARG = -1          # include/cpg_hip.h
_ip = C.POINTER(C.c_int32)


def _nnls(m, n):
    """tests/test_gradient.py, test_adjoint_kernel_vs_oracle_emulator: every parameter perturbed by 5 %, rng 1"""
    def make(B):
        d = families.nonneg_ls(m, n, sparsity=None, seed=0)
        rng = np.random.default_rng(1)
        th = np.tile(d.theta0, (B, 1))
        th[:, :d.NP] *= 1 + 0.05 * rng.standard_normal((B, d.NP))
        vals = {p.name: th[:, p.col:p.col + p.size] for p in d.params}
        return d, vals, None, th, dict(eps_abs=1e-4, eps_rel=1e-4, max_iter=100), 1e-10
    return make


def _mpc(B):
    """tests/test_gradient.py, test_adjoint_on_the_pruned_factor_pattern: only x_init varies, rng 6"""
    d = families.mpc(4, 2, 3)
    rng = np.random.default_rng(6)
    x0 = -2 + 4 * rng.random((B, 4))
    th = np.tile(d.theta0, (B, 1))
    p = d.param('x_init')
    th[:, p.col:p.col + p.size] = x0
    return d, {'x_init': x0}, ['x_init'], th, dict(eps_abs=1e-6, eps_rel=1e-6), 1e-8


FAMILIES = {'nnls_10x5': _nnls(10, 5), 'nnls_1x1': _nnls(1, 1), 'mpc_4_2_3': _mpc}


def _upstream(d, B):
    """loss = 0.1 * sum(variables) (tests/test_diff.py:38), made instance- and entry-dependent so that a scatter to the wrong
    place or instance shows"""
    rng = np.random.default_rng(3)
    return {v.name: 0.1 * (1 + rng.random((B,) + tuple(v.shape))) for v in d.variables}


def _canonical_dx(d, dv, B):
    dx = np.zeros((B, d.n_var))
    for v in d.variables:
        g = dv[v.name]
        dx[:, v.indices] = g.transpose((0,) + tuple(range(len(v.shape), 0, -1))).reshape(B, -1) if len(v.shape) > 1 else g.reshape(B, -1)
    return dx


def _run(lib_path, family, B, canonical):
    """forward into a DeviceBatch, adjoint queued at once (after = the solving handle), ONLY the gradient handle waited for;
    then the host entry point on the solution the device buffers hold.  Returns everything the checks need."""
    d, vals, upd, th, settings, tol = FAMILIES[family](B)
    bs = BatchSolver(d, lib_path=lib_path, full_output=True)
    try:
        bs.set_updated(upd)
        bs.apply_settings(**settings)
        dev, gdev = DeviceBatch(bs, B), DeviceGradBatch(bs, B, canonical=canonical)
        dv = _upstream(d, B)
        # a warm step on other inputs first: the gradient handle, its factor plan, adjoint tables and variable table are
        # loaded and the scratch is allocated, so that in the step under test nothing but two launches lies between the
        # solve and the adjoint -- the event wait alone keeps the adjoint from reading a solution that is not there yet
        tv = bs.theta_var(vals)
        gdev.upload_dvars(np.zeros((B, gdev.n_dvars)))
        dev.upload(np.ascontiguousarray(tv[::-1]) * 0.5)
        bs.solve_device(dev)
        bs.gradient_device(dev, gdev)
        gdev.synchronize()
        gdev.upload_dvars(_canonical_dx(d, dv, B) if canonical else dv)
        dev.upload(tv)
        bs.solve_device(dev)
        bs.gradient_device(dev, gdev)                      # no synchronize() in between
        g_dev = gdev.download()                            # waits for the gradient handle's stream only
        ms = gdev.last_kernel_ms()
        h_dev = bs.h_grad
        r = dev.download()
        g_host = bs.gradient(vals, r.sol_x, r.sol_y, dv, updated_params=upd)
        assert bs.h_grad is h_dev                          # the device path picked the handle gradient() picks
        dev.free(); gdev.free()
        return dict(d=d, th=th, r=r, dv=dv, g_dev=g_dev, g_host=g_host, tol=tol, ms=ms, pruned=h_dev is bs.h_rg)
    finally:
        bs.close()


def _check_against_host(c, B):
    d = c['d']
    assert c['g_dev']['_flat'].shape == (B, d.NP)
    assert np.isfinite(c['g_host']['_flat']).all() and np.abs(c['g_host']['_flat']).max() > 1e-4
    assert sorted(c['g_dev']) == sorted(c['g_host'])
    for k in c['g_host']:
        assert c['g_dev'][k].shape == c['g_host'][k].shape and np.array_equal(c['g_dev'][k], c['g_host'][k]), k
    assert c['ms'] >= 0.0


def _check_against_oracle(c, B, oracle_lib):
    """per instance, the bound of tests/test_gradient.py: 1e-10 |dtheta|_max on nonneg-LS, 1e-8 max(1, |dtheta|_max) on the MPC
    adjoint.  An instance whose variables all sit on their bound has gradient ZERO (the active rows absorb the whole upstream
    gradient): the oracle returns rounding noise there (~1e-19 next to ~1e-2 for the others) and a bound relative to that noise
    cannot be met by anything.  Such an instance -- told by the oracle alone: its |dtheta|_max is below 1e-12 of the batch's --
    must come out of the kernel as zero on the batch's scale: |g_dev| <= tol * the batch's largest gradient."""
    d, r = c['d'], c['r']
    dx = _canonical_dx(d, c['dv'], B)
    big = c['tol'] == 1e-8
    G = np.array([oracle_lib.qp_adjoint(d, d.canon_at(c['th'][k]), r.sol_x[k], r.sol_y[k], dx[k])['dtheta'] for k in range(B)])
    batch = np.abs(G).max()
    assert batch > 1e-4
    for k in range(B):
        scale = np.abs(G[k]).max()
        if scale < 1e-12 * batch:
            assert np.abs(c['g_dev']['_flat'][k]).max() <= c['tol'] * batch, k
        else:
            assert np.abs(c['g_dev']['_flat'][k] - G[k]).max() <= c['tol'] * (max(1.0, scale) if big else scale), k


@pytest.fixture(scope='module')
def sim_case(sim_lib):
    cache = {}

    def get(family, B, canonical):
        key = (family, B, canonical)
        if key not in cache:
            cache[key] = _run(sim_lib, family, B, canonical)
        return cache[key]
    return get


# B = 70: more than one pass of the wavefronts the emulator's launch keeps resident, and no multiple of the workgroup width
@pytest.mark.parametrize('canonical', [False, True], ids=['table', 'canonical'])
@pytest.mark.parametrize('B', [1, 3, 70])
@pytest.mark.parametrize('family', list(FAMILIES))
def test_device_adjoint_equals_host_adjoint_emulator(sim_case, family, B, canonical):
    c = sim_case(family, B, canonical)
    _check_against_host(c, B)
    assert c['pruned'] == (family == 'mpc_4_2_3')


@pytest.mark.parametrize('B', [1, 3, 70])
@pytest.mark.parametrize('family', list(FAMILIES))
def test_device_adjoint_vs_oracle_emulator(sim_case, oracle_lib, family, B):
    _check_against_oracle(sim_case(family, B, False), B, oracle_lib)


# ---- raw C-ABI ------------------------------------------------------------------------------------------------------
class _Raw:
    """device buffers and calls of the C-ABI on one gradient handle, every buffer sized from the family"""

    def __init__(self, bs, hg):
        self.bs, self.L, self.hg, self.bufs = bs, bs.lib.L, hg, []

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = C.c_void_p()
        self.bs.lib.check(self.L.cpg_hip_malloc(self.hg, max(a.nbytes, 8), C.byref(p)), 'malloc')
        self.bufs.append(p)
        if a.nbytes:
            self.bs.lib.check(self.L.cpg_hip_memcpy_h2d(self.hg, p, a.ctypes.data_as(C.c_void_p), a.nbytes), 'h2d')
        return p

    def set_vars(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        return self.L.cpg_hip_set_gradient_vars(self.hg, len(idx), idx.ctypes.data_as(_ip) if len(idx) else None)

    def gradient(self, B, tv, sx, sy, dvars, NP, after=None):
        out = self.put(np.full((B, NP), np.nan))
        rc = self.L.cpg_hip_gradient_batch_device(self.hg, B, self.put(tv), self.put(sx), self.put(sy), self.put(dvars), out, after)
        if rc:
            return rc, None
        self.bs.lib.check(self.L.cpg_hip_synchronize(self.hg), 'sync')
        dth = np.empty((B, NP))
        self.bs.lib.check(self.L.cpg_hip_memcpy_d2h(self.hg, dth.ctypes.data_as(C.c_void_p), out, dth.nbytes), 'd2h')
        return 0, dth

    def free(self):
        for p in self.bufs:
            self.L.cpg_hip_free(self.hg, p)


def test_duplicate_table_entries_accumulate_deterministically(sim_lib):
    """a 2 x 2 symmetric variable over three canonical entries: user entries (F order) 00, 10, 01, 11 -> i0, i1, i1, i2"""
    B = 3
    d, vals, upd, th, settings, _ = FAMILIES['nnls_10x5'](B)
    bs = BatchSolver(d, lib_path=sim_lib, full_output=True)
    r = bs.solve(vals, **settings)
    xi = d.variables[0].indices
    table = np.array([xi[0], xi[1], xi[1], xi[2]], dtype=np.int32)
    rng = np.random.default_rng(4)
    dvars = 0.1 * (1 + rng.random((B, 4)))
    dx = np.zeros((B, d.n_var))
    dx[:, xi[0]], dx[:, xi[1]], dx[:, xi[2]] = dvars[:, 0], dvars[:, 1] + dvars[:, 2], dvars[:, 3]
    g_host = bs.gradient(vals, r.sol_x, r.sol_y, {'x': dx[:, xi]})['_flat']      # the pre-summed canonical dx
    raw = _Raw(bs, bs.h_grad)
    assert raw.set_vars(table) == 0
    tv = bs.theta_var(vals, names=[q.name for q in d.params])
    rc1, g1 = raw.gradient(B, tv, r.sol_x, r.sol_y, dvars, d.NP)
    rc2, g2 = raw.gradient(B, tv, r.sol_x, r.sol_y, dvars, d.NP, after=bs.h_grad)     # after == h: orders nothing
    assert rc1 == 0 and rc2 == 0
    assert np.array_equal(g1, g2)
    assert np.abs(g1 - g_host).max() <= 1e-15 * np.abs(g_host).max()
    # the table is sticky until replaced; n_gv = 0 goes back to the canonical layout
    assert raw.set_vars([]) == 0
    rc3, g3 = raw.gradient(B, tv, r.sol_x, r.sol_y, dx, d.NP)
    assert rc3 == 0 and np.array_equal(g3, g_host)
    assert raw.gradient(0, tv, r.sol_x, r.sol_y, dx, d.NP)[0] == 0              # B == 0: CPG_OK, nothing to do
    raw.free()
    bs.close()


def test_refusals(sim_lib):
    B = 3
    d, vals, upd, th, settings, _ = FAMILIES['nnls_10x5'](B)
    # a solver without the canonical solution
    bs0 = BatchSolver(d, lib_path=sim_lib)
    bs0.set_updated(upd)
    dev0, gdev0 = DeviceBatch(bs0, B), DeviceGradBatch(bs0, B)
    with pytest.raises(ValueError, match='full_output'):
        bs0.gradient_device(dev0, gdev0)
    assert not bs0._grad_loaded_on                               # no handle was given adjoint tables
    dev0.free(); gdev0.free(); bs0.close()

    bs = BatchSolver(d, lib_path=sim_lib, full_output=True)
    bs.set_updated(upd)
    dev, gdev2 = DeviceBatch(bs, B), DeviceGradBatch(bs, B - 1)
    with pytest.raises(ValueError, match='batch sizes'):
        bs.gradient_device(dev, gdev2)
    assert not bs._grad_loaded_on
    with pytest.raises(ValueError, match=r'shape \(2, 5\)'):
        gdev2.upload_dvars(np.zeros((B, 5)))
    with pytest.raises(RuntimeError, match='no adjoint'):
        gdev2.download()
    # a DeviceBatch of another parameter set
    gdev = DeviceGradBatch(bs, B)
    bs.set_updated(['b'])
    with pytest.raises(ValueError, match='updated parameters changed'):
        bs.gradient_device(dev, gdev)
    bs.set_updated(upd)

    # C-ABI: the device entry point and the table need cpg_hip_set_gradient on the handle
    bs._set_refactor(bs._var_cols, bs._th_fixed)
    raw = _Raw(bs, bs.h_ref)
    z = np.zeros((B, max(d.n_var, d.m, d.NP)))
    rc, _ = raw.gradient(B, z[:, :d.NP], z[:, :d.n_var], z[:, :d.m], z[:, :d.n_var], d.NP)
    assert rc == CPG_E_BADARG and b'cpg_hip_set_gradient' in bs.lib.L.cpg_hip_last_error()
    assert raw.set_vars([0]) == CPG_E_BADARG
    # ... and the table's indices must lie in [0, n)
    bs._set_gradient(bs.h_ref)
    for bad in ([0, d.n_var], [-1], [1, 2, 1 << 20]):
        assert raw.set_vars(bad) == CPG_E_BADARG, bad
        assert b'outside' in bs.lib.L.cpg_hip_last_error()
    assert raw.set_vars([0, d.n_var - 1]) == 0
    # null buffers are refused as by cpg_hip_gradient_batch
    assert bs.lib.L.cpg_hip_gradient_batch_device(bs.h_ref, B, None, None, None, None, None, None) == CPG_E_BADARG
    raw.free(); dev.free(); gdev.free(); gdev2.free(); bs.close()


def test_shim_device_training_step(sim_lib, tmp_path):
    """GeneratedSolver.cpg_solve_and_gradient_device: forward and backward through the device objects, equal to
    cpg_solve_batch + cpg_gradient_batch; the second step reuses the buffers"""
    from cvxpygen_amd import cpg
    from cvxpygen_amd.lite import LiteProblem
    d = families.nonneg_ls()
    prob = LiteProblem.from_descriptor(d)
    cpg.generate_code(prob, code_dir=str(tmp_path / 'dev_code'), solver='OSQP', gradient=True, wrapper=False)   # (no hipcc step: the emulator library is injected)
    mod = cpg.load_generated(str(tmp_path / 'dev_code'), prob)
    mod._SOLVER.lib_path = sim_lib
    B = 3
    rng = np.random.default_rng(12)
    for step in range(2):
        params = {'A': rng.standard_normal((B, 3)), 'b': rng.standard_normal((B, 3))}
        up = 0.1 * (1 + rng.random((B, 2)))
        dev, gdev = mod.cpg_solve_and_gradient_device(params, lambda dev, gdev: {'x': up}, eps_abs=1e-9, eps_rel=1e-9)
        g = gdev.download()
        r = dev.download()
        assert (r.status == 1).all()
        r2 = mod.cpg_solve_batch(params, eps_abs=1e-9, eps_rel=1e-9)
        assert np.array_equal(r.sol_x, r2.sol_x) and np.array_equal(r.sol_y, r2.sol_y)
        g2 = mod.cpg_gradient_batch(params, r2.sol_x, r2.sol_y, {'x': up})
        for k in g2:
            assert np.array_equal(g[k], g2[k]), (step, k)
    assert mod._SOLVER._dev_step[1] is dev
    mod._SOLVER.free_device_step()
    assert mod._SOLVER._dev_step is None
    # a solver without the canonical solution on the device (as the two-stage and conic ones) is refused up front
    mod._SOLVER.batch_solver.full_output = False
    with pytest.raises(ValueError, match='device-resident step'):
        mod.cpg_solve_and_gradient_device(params, lambda dev, gdev: None)
    mod._SOLVER.batch_solver.full_output = True


# ---- GPU tier -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu_case():
    cache = {}

    def get(family, B, canonical):
        key = (family, B, canonical)
        if key not in cache:
            cache[key] = _run(None, family, B, canonical)
        return cache[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize('canonical', [False, True], ids=['table', 'canonical'])
@pytest.mark.parametrize('B', [3, 1000])
@pytest.mark.parametrize('family', list(FAMILIES))
def test_device_adjoint_equals_host_adjoint_gpu(gpu_case, family, B, canonical):
    """also the ordering check: the adjoint is queued behind the forward solve of another handle with no host
    synchronisation, and a solution read too early would not reproduce the host path bit for bit"""
    c = gpu_case(family, B, canonical)
    _check_against_host(c, B)
    assert c['ms'] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('B', [3, 1000])
@pytest.mark.parametrize('family', list(FAMILIES))
def test_device_adjoint_vs_oracle_gpu(gpu_case, oracle_lib, family, B):
    _check_against_oracle(gpu_case(family, B, False), B, oracle_lib)

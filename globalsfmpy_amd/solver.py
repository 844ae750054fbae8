"""Flat-array host API over the C-ABI (include/gsfm_rot.h).

`RotationProblem` is the numpy-facing wrapper used by bench.py, the tests and the
GlobalSfMpy-compatible estimator classes.  It owns one `gsfm_rot_problem`.
"""
import ctypes as C
import numpy as np

from . import _abi


_CTYPES = {np.dtype(t): c for t, c in ((np.float64, C.c_double), (np.uint8, C.c_uint8), (np.int32, C.c_int32), (np.uint32, C.c_uint32),
                                      (np.int64, C.c_int64), (np.uint64, C.c_uint64))}


def _p(a):
    """The ctypes pointer to a contiguous array's data, typed by the array's dtype; None passes through as NULL."""
    return None if a is None else a.ctypes.data_as(C.POINTER(_CTYPES[a.dtype]))


_dp = _u32p = _p   # the older names, which oracle/pyoracle.py imports


class SolverError(RuntimeError):
    pass


def _raise_if_failed(lib, name, st):
    """The one error path of the calls that take no problem object: `name` is the C entry point, `st` its status."""
    if st != 0:
        raise SolverError("%s failed with status %d: %s" % (name, st, lib.gsfm_last_error().decode("utf-8", "replace")))


def _loss_nodes(loss, who, callback_ok=False):
    """A loss argument as a list of (kind, p0, p1, p2) nodes: None (Ceres' NULL loss), such a list, or an object with .native_program().
    callback_ok: an object that has only .Evaluate gives None (the caller takes the host callback path); otherwise `who` needs a native loss."""
    if loss is None:
        return []
    if isinstance(loss, (list, tuple)):
        return list(loss)
    if hasattr(loss, "native_program") and loss.native_program() is not None:
        return loss.native_program()
    if not callback_ok:
        raise TypeError("the %s needs a loss with a native descriptor, got %r" % (who, loss))
    if hasattr(loss, "Evaluate"):
        return None
    raise TypeError("unsupported loss object %r" % (loss,))


class _Handle(object):
    """The lifetime of a problem handle (self._lib, self._h, destroyed by the entry self._prefix + "problem_destroy") and the options of a
    solve by name (the subclass's default_options())."""
    _prefix = None
    _h = None

    def _fn(self, name):
        return getattr(self._lib, self._prefix + name)

    def close(self):
        if self._h is not None:
            self._fn("problem_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _options(self, kw):
        o = self.default_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise TypeError("unknown solver option %r" % k)
            setattr(o, k, v)
        return o


class ProblemBase(_Handle):
    """Shared call sequence for anything exporting the gsfm_rot_* argument lists.
    (The CPU oracle under oracle/ mirrors them with an orc_ prefix for the parity tests.)"""

    _prefix = "gsfm_rot_"

    def __init__(self, lib, handle, n_cams, n_edges, error_type, residual_dim):
        self._lib = lib
        self._h = handle
        self.n_cams = int(n_cams)
        self.n_edges = int(n_edges)
        self.error_type = int(error_type)
        self.residual_dim = int(residual_dim)
        self._keep = []

    def _check(self, st, what):
        # every C call may have run the host-callback loss: an exception parked by the trampoline surfaces HERE, from the call that caused
        # it, not from some later, unrelated one
        self._reraise_callback_error()
        if st != 0:
            raise SolverError("%s failed with status %d: %s" % (what, st, self._last_error()))
        comm = getattr(self, "_comm", None)
        if comm is not None and hasattr(comm, "take_error") and comm.take_error():
            # (peer-store exchange: a wait for a peer's slice timed out in the last calls of this solve -- what it returned is not a result;
            # the captured PCG chunks still hold the peer kernels: set_stream drops them, the next solve captures the fallback's)
            self._lib.gsfm_rot_set_stream(self._h, C.c_void_p(comm.stream_handle() or 0))
            raise SolverError("%s: the peer-store exchange timed out waiting for a peer; the result is invalid (later solves use the fallback collectives)" % what)

    def _last_error(self):
        return ""

    # -- loss ---------------------------------------------------------------
    def set_loss(self, loss):
        """loss: None (Ceres NULL loss), a list of (kind, p0, p1, p2) nodes, or an object with
        .native_program() (globalsfmpy_amd.loss_functions classes); any other object with
        .Evaluate(s, out) is used through the host callback path."""
        nodes = _loss_nodes(loss, None, callback_ok=True)
        if nodes is None:
            return self.set_loss_callback(loss.Evaluate)
        arr, n = _abi.make_program(nodes)
        self._check(self._fn("set_loss")(self._h, arr, n), "set_loss")

    def set_loss_callback(self, evaluate):
        """Host-callback loss.  An exception raised by `evaluate` cannot cross the C boundary: it is recorded, the edge gets NaN
        (the solve then ends with FAILURE / nonfinite instead of running on stale values) and solve() re-raises it."""
        self._cb_error = None

        def _cb(_user, s, out):
            try:
                buf = [0.0, 0.0, 0.0]
                evaluate(s, buf)
                out[0], out[1], out[2] = buf[0], buf[1], buf[2]
            except BaseException as e:  # noqa: BLE001
                if self._cb_error is None:
                    self._cb_error = e
                out[0] = out[1] = out[2] = float("nan")
        cb = _abi.LOSS_CALLBACK_FN(_cb)
        self._keep.append(cb)
        self._check(self._fn("set_loss_callback")(self._h, cb, None), "set_loss_callback")

    def _reraise_callback_error(self):
        e, self._cb_error = getattr(self, "_cb_error", None), None
        if e is not None:
            raise e

    def set_edge_weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert w.shape == (self.n_edges,)
        self._check(self._fn("set_edge_weights")(self._h, _p(w)), "set_edge_weights")

    # -- evaluation ---------------------------------------------------------
    def residuals(self, rot_aa, want_residuals=False):
        rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(self.n_cams, 3)
        s = np.empty(self.n_edges)
        rho = np.empty((self.n_edges, 3))
        r = np.empty((self.n_edges, self.residual_dim)) if want_residuals else None
        cost = C.c_double(0)
        st = self._fn("residuals")(self._h, _p(rot), _p(s), _p(rho), _p(r), C.byref(cost))
        self._check(st, "residuals")
        return {"s": s, "rho": rho, "residuals": r, "cost": cost.value}

    def linearize(self, rot_aa):
        rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(self.n_cams, 3)
        g = np.empty((self.n_cams, 3))
        d = np.empty((self.n_cams, 3, 3))
        cost = C.c_double(0)
        self._check(self._fn("linearize")(self._h, _p(rot), _p(g), _p(d), C.byref(cost)), "linearize")
        return {"gradient": g, "diag_blocks": d, "cost": cost.value}

    def normal_matvec(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(self.n_cams, 3)
        y = np.empty_like(v)
        self._check(self._fn("normal_matvec")(self._h, _p(v), _p(y)), "normal_matvec")
        return y

    # -- solve --------------------------------------------------------------
    def default_options(self):
        o = _abi.Options()
        self._options_default(o)
        return o

    def solve(self, rot_aa, **options):
        rot = np.array(rot_aa, dtype=np.float64, order="C").reshape(self.n_cams, 3)
        o = self._options(options)
        s = _abi.Summary()
        st = self._fn("solve")(self._h, _p(rot), C.byref(o), C.byref(s))
        self._check(st, "solve")
        return rot, s.as_dict()

    def solve_sigma_consensus(self, rot_aa, iters_num, sigma_max, **options):
        rot = np.array(rot_aa, dtype=np.float64, order="C").reshape(self.n_cams, 3)
        o = self._options(options)
        s = _abi.Summary()
        st = self._fn("solve_sigma_consensus")(self._h, _p(rot), int(iters_num), float(sigma_max), C.byref(o), C.byref(s))
        self._check(st, "solve_sigma_consensus")
        return rot, s.as_dict()

    def trace(self):
        rows = self._fn("get_trace")(self._h, None, 0)
        out = np.zeros((max(rows, 0), 8))
        if rows > 0:
            self._fn("get_trace")(self._h, _p(out), rows)
        return out


def _device_rotations(rot_dev, n_cams):
    """Device address of a (n_cams, 3) float64 buffer: a contiguous torch CUDA tensor, anything with __cuda_array_interface__, or an int."""
    if isinstance(rot_dev, int):
        return rot_dev
    if hasattr(rot_dev, "data_ptr"):   # torch
        if not rot_dev.is_cuda or str(rot_dev.dtype) != "torch.float64" or not rot_dev.is_contiguous() or rot_dev.numel() != 3 * n_cams:
            raise ValueError("solve_resident needs a contiguous float64 CUDA tensor of %d x 3" % n_cams)
        return int(rot_dev.data_ptr())
    cai = getattr(rot_dev, "__cuda_array_interface__", None)
    if cai is None:
        raise TypeError("solve_resident needs device memory (a torch CUDA tensor, __cuda_array_interface__ or a raw address); host arrays go to solve()")
    if cai["typestr"] not in ("<f8", "=f8") or int(np.prod(cai["shape"])) != 3 * n_cams or cai.get("strides") is not None:
        raise ValueError("solve_resident needs a contiguous float64 device buffer of %d x 3" % n_cams)
    return int(cai["data"][0])


def _prep_edges(n_cams, edge_i, edge_j, rel_aa, cov6, inlier_weight):
    ei = np.ascontiguousarray(edge_i, dtype=np.uint32)
    ej = np.ascontiguousarray(edge_j, dtype=np.uint32)
    rel = np.ascontiguousarray(rel_aa, dtype=np.float64).reshape(-1, 3)
    n_edges = ei.shape[0]
    if ej.shape[0] != n_edges or rel.shape[0] != n_edges:
        raise ValueError("edge arrays disagree in length")
    c6 = None if cov6 is None else np.ascontiguousarray(cov6, dtype=np.float64).reshape(n_edges, 6)
    iw = None if inlier_weight is None else np.ascontiguousarray(inlier_weight, dtype=np.float64).reshape(n_edges)
    return ei, ej, rel, c6, iw, n_edges


class RotationProblem(ProblemBase):
    """The product: gsfm_rot_problem on the current HIP device."""

    def __init__(self, n_cams, edge_i, edge_j, rel_aa, error_type=_abi.ANGLE_AXIS, cov6=None,
                 inlier_weight=None, shard=None, stream=None):
        lib = _abi.load_library()
        ei, ej, rel, c6, iw, n_edges = _prep_edges(n_cams, edge_i, edge_j, rel_aa, cov6, inlier_weight)
        h = C.c_void_p()
        st = lib.gsfm_rot_problem_create(int(n_cams), int(n_edges), _p(ei), _p(ej), _p(rel), int(error_type),
                                         _p(c6), _p(iw), C.byref(shard) if shard is not None else None, C.byref(h))
        _raise_if_failed(lib, "gsfm_rot_problem_create", st)
        ProblemBase.__init__(self, lib, h, n_cams, n_edges, error_type, lib.gsfm_rot_residual_dim(int(error_type)))
        self._shard = shard
        if stream is not None:
            self._check(lib.gsfm_rot_set_stream(self._h, C.c_void_p(int(stream))), "set_stream")

    def _last_error(self):
        return self._lib.gsfm_last_error().decode("utf-8", "replace")

    def _options_default(self, o):
        self._lib.gsfm_rot_options_default(C.byref(o))

    def solve_resident(self, rot_dev, **options):
        """gsfm_rot_solve_resident: `rot_dev` is DEVICE memory on the problem's device ((n_cams, 3) float64, contiguous: a torch CUDA tensor,
        an object with __cuda_array_interface__, or a raw address), read as the start and overwritten with the result -- nothing but the
        summary crosses PCIe.  Returns the summary; the stream is synchronised on return."""
        ptr = _device_rotations(rot_dev, self.n_cams)
        o = self._options(options)
        s = _abi.Summary()
        st = self._lib.gsfm_rot_solve_resident(self._h, C.c_void_p(ptr), C.byref(o), C.byref(s))
        self._check(st, "solve_resident")
        return s.as_dict()

    def step_check(self, rot_aa, radius=1e4, loose_tau=0.0, **options):
        """gsfm_rot_step_check (a testing aid): one LM step's linear algebra at rot_aa, as iteration 1 of a solve from there at `radius`, by the
        solve's own phases.  Returns a dict: eta, delta (n x 3), x, x_trial (n x 3, or n x 4 for the quaternion types), lam (n x 3), the
        fields of gsfm_rot_step_info (path, cg_iterations, cg_rel, cg_tolerance, coarse_n, lin_is_lap, column_sorted, graph_launches,
        dense_info, gmax, cost, step_sums), model_cost_change from the step's sums, and with loose_tau > 0 on a PCG-solved step eta_loose,
        delta_loose, loose_cg_iterations, loose_cg_rel (None / -1 otherwise)."""
        rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(self.n_cams, 3)
        o = self._options(options)
        n = self.n_cams
        pd = 3 if self.error_type in (_abi.ANGLE_AXIS_COVARIANCE, _abi.ANGLE_AXIS, _abi.ANGLE_AXIS_INLIERS, _abi.ANGLE_AXIS_COV_INLIERS,
                                      _abi.ANGLE_AXIS_COVTRACE, _abi.ANGLE_AXIS_COVNORM) else 4
        eta, delta, lam, xs, xt = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, pd)), np.zeros((n, pd))
        eta_l, delta_l = np.zeros((n, 3)), np.zeros((n, 3))
        info = _abi.StepInfo()
        st = self._lib.gsfm_rot_step_check(self._h, _p(rot), float(radius), float(loose_tau), C.byref(o), _p(eta), _p(delta), _p(xs), _p(xt), _p(lam),
                                           _p(eta_l), _p(delta_l), C.byref(info))
        self._check(st, "step_check")
        out = {name: getattr(info, name) for name, _ in info._fields_}
        out["step_sums"] = np.array(list(info.step_sums))
        s = out["step_sums"]
        out["model_cost_change"] = -0.5 * s[0] + 0.5 * s[1] + 0.5 * s[2]
        loose = info.loose_cg_iterations >= 0
        out.update(eta=eta, delta=delta, x=xs, x_trial=xt, lam=lam, eta_loose=eta_l if loose else None, delta_loose=delta_l if loose else None)
        return out

    def time_sweep(self, rot_aa, reps=20):
        rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(self.n_cams, 3)
        ms = C.c_double(0)
        self._check(self._lib.gsfm_rot_time_sweep(self._h, _p(rot), int(reps), C.byref(ms)), "time_sweep")
        return ms.value

    def time_kernels(self, rot_aa, reps=10):
        """Mean HIP-event time (ms) of k_cost, the linearisation and one mat-vec (row-major or column-sorted forms, incl. their finish kernels)."""
        rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(self.n_cams, 3)
        out = np.zeros(4)
        self._check(self._lib.gsfm_rot_time_kernels(self._h, _p(rot), int(reps), _p(out)), "time_kernels")
        return {"k_cost": out[0], "k_lin": out[1], "k_matvec": out[2]}

    def matvec_bytes(self):
        """(bytes one mat-vec streams as laid out, form: 0 general blocks, 1 Laplacian row-major, 2 Laplacian column-sorted)."""
        b, l, f = C.c_double(0), C.c_double(0), C.c_int32(0)
        self._check(self._lib.gsfm_rot_matvec_bytes(self._h, C.byref(b), C.byref(l), C.byref(f)), "matvec_bytes")
        return b.value, int(f.value)

    def linearize_bytes(self):
        b, l, f = C.c_double(0), C.c_double(0), C.c_int32(0)
        self._check(self._lib.gsfm_rot_matvec_bytes(self._h, C.byref(b), C.byref(l), C.byref(f)), "matvec_bytes")
        return l.value

    def loss_eval(self, s, with_fast_rho1=False):
        """(rho, rho', rho'')(s) and the cost-only rho(s) of the current native loss, evaluated by the device routines; with_fast_rho1 adds
        rho'(s) as the fast path of the linearisation K2 computes it (NaN for loss programs that have no fast path)."""
        s = np.ascontiguousarray(s, dtype=np.float64).ravel()
        rho3, val = np.empty((s.size, 3)), np.empty(s.size)
        fast = np.empty(s.size) if with_fast_rho1 else None
        self._check(self._lib.gsfm_rot_loss_eval(self._h, _p(s), s.size, _p(rho3), _p(val), _p(fast)), "loss_eval")
        return (rho3, val, fast) if with_fast_rho1 else (rho3, val)

    def edge_order(self):
        """order[u] = index (in the arrays given at creation) of the edge at position u of the device-side per-edge planes."""
        n = self._lib.gsfm_rot_edge_order(self._h, None, 0)
        out = np.empty(max(n, 0), dtype=np.uint32)
        if n > 0:
            self._lib.gsfm_rot_edge_order(self._h, _p(out), n)
        return out

    def time_sweep_variants(self, rot_aa, reps=10):
        """Mean HIP-event time (ms) of the K1 variants (trial cost; s + rho triple stored; s only; rho' only) and of the sigma-consensus
        forms of K1 / K2 against their plain forms (zeros unless the problem is an ANGLE_AXIS one carrying scalar weights)."""
        rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(self.n_cams, 3)
        out = np.zeros(8)
        self._check(self._lib.gsfm_rot_time_sweep_variants(self._h, _p(rot), int(reps), _p(out)), "time_sweep_variants")
        return {"trial_cost": out[0], "full_reweight": out[1], "s_only": out[2], "rho1_only": out[3],
                "k1_sigma_fused": out[4], "k1_sigma_plain": out[5], "k2_sigma_fused": out[6], "k2_sigma_plain": out[7]}

    def sweep_bytes(self):
        a, b = C.c_double(0), C.c_double(0)
        self._check(self._lib.gsfm_rot_sweep_bytes(self._h, C.byref(a), C.byref(b)), "sweep_bytes")
        return a.value, b.value


def magsac_table(nu):
    lib = _abi.load_library()
    n = lib.gsfm_magsac_table(int(nu), None, 0)
    out = np.empty(n)
    lib.gsfm_magsac_table(int(nu), _p(out), n)
    return out


def magsac_constants(nu):
    lib = _abi.load_library()
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    lib.gsfm_magsac_constants(int(nu), C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def edge_sq_norms(n_cams, edge_i, edge_j, rel_aa, rot_aa, cov6=None, max_sq_norm=None):
    """gsfm_rot_edge_sq_norms: per-edge squared (whitened) loop residual on the device, and the keep mask of the orientation filter."""
    lib = _abi.load_library()
    ei, ej, rel, c6, _, n_edges = _prep_edges(n_cams, edge_i, edge_j, rel_aa, cov6, None)
    rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(int(n_cams), 3)
    s = np.empty(n_edges)
    keep = np.empty(n_edges, dtype=np.uint8) if max_sq_norm is not None else None
    kept, ms = C.c_uint64(0), C.c_double(0)
    st = lib.gsfm_rot_edge_sq_norms(int(n_cams), int(n_edges), _p(ei), _p(ej), _p(rel), _p(c6), _p(rot),
                                    float(max_sq_norm if max_sq_norm is not None else -1.0), _p(s),
                                    _p(keep), C.byref(kept), C.byref(ms))
    _raise_if_failed(lib, "gsfm_rot_edge_sq_norms", st)
    return {"s": s, "keep": None if keep is None else keep.astype(bool), "n_kept": int(kept.value), "kernel_ms": ms.value}


def orientations_from_maximum_spanning_tree(n_cams, edge_i, edge_j, rel_aa, weight=None):
    """gsfm_rot_init_spanning_tree: theia's OrientationsFromMaximumSpanningTree on flat arrays, on the device.  The maximum spanning
    tree of the largest connected component under (weight desc, edge index asc), rooted at the component's smallest camera, rotations
    composed down it (R_j = R_ij R_i across edge (i, j)).  weight: per-edge num_verified_matches (int32), None = all equal.
    Returns dict(rot_aa (n_cams x 3, zeros outside the component), parent_edge (int64 per camera, -1 for the root and outside),
    root, n_tree_cams, depth, kernel_ms)."""
    lib = _abi.load_library()
    ei, ej, rel, _, _, n_edges = _prep_edges(n_cams, edge_i, edge_j, rel_aa, None, None)
    wt = None
    if weight is not None:
        wt = np.ascontiguousarray(weight, dtype=np.int32).reshape(-1)
        if wt.shape[0] != n_edges:
            raise ValueError("weight disagrees with the edges in length")
    n = int(n_cams)
    rot = np.empty((n, 3))
    parent = np.empty(n, dtype=np.int64)
    root, n_tree, depth, ms = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_double(0)
    st = lib.gsfm_rot_init_spanning_tree(n, int(n_edges), _p(ei), _p(ej), _p(rel),
                                         _p(wt), _p(rot),
                                         _p(parent), C.byref(root), C.byref(n_tree), C.byref(depth), C.byref(ms))
    _raise_if_failed(lib, "gsfm_rot_init_spanning_tree", st)
    return {"rot_aa": rot, "parent_edge": parent, "root": int(root.value), "n_tree_cams": int(n_tree.value), "depth": int(depth.value),
            "kernel_ms": ms.value}


def _rot_l1l2_options(lib, kw):
    o = _abi.RotL1L2Options()
    lib.gsfm_rot_l1l2_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k) or k == "reserved_":
            raise TypeError("unknown option %r of the robust rotation estimator" % k)
        setattr(o, k, v)
    return o


def _rot_l1l2_edges(edge_i, edge_j, rel_aa):
    ei = np.ascontiguousarray(edge_i, dtype=np.uint32).reshape(-1)
    ej = np.ascontiguousarray(edge_j, dtype=np.uint32).reshape(-1)
    rel = None if rel_aa is None else np.ascontiguousarray(rel_aa, dtype=np.float64).reshape(-1, 3)
    if ej.shape[0] != ei.shape[0] or (rel is not None and rel.shape[0] != ei.shape[0]):
        raise ValueError("edge_i, edge_j and rel_aa must describe the same edges")
    return ei, ej, rel


def estimate_rotations_robust_l1l2(n_cams, edge_i, edge_j, rel_aa, init_aa, fixed_cam=0, **options):
    """gsfm_rot_l1l2_solve: Theia's RobustRotationEstimator (ROBUST_L1L2: L1 by ADMM, then IRLS) under the definition of
    include/gsfm_rot_l1l2.h, on the device.  Edges are used as listed (i > j and repeated pairs allowed); init_aa: n_cams x 3 start
    rotations; fixed_cam: the camera held constant.  options: the fields of gsfm_rot_l1l2_options.  Returns (rot_aa, summary dict)."""
    lib = _abi.load_library()
    n = int(n_cams)
    ei, ej, rel = _rot_l1l2_edges(edge_i, edge_j, rel_aa)
    rot = np.array(init_aa, dtype=np.float64, order="C").reshape(n, 3)
    o = _rot_l1l2_options(lib, options)
    s = _abi.RotL1L2Summary()
    st = lib.gsfm_rot_l1l2_solve(n, ei.shape[0], _p(ei), _p(ej), _p(rel), _p(rot), int(fixed_cam), C.byref(o), C.byref(s))
    _raise_if_failed(lib, "gsfm_rot_l1l2_solve", st)
    return rot, s.as_dict()


def robust_l1l2_residuals(n_cams, edge_i, edge_j, rel_aa, rot_aa, **options):
    """gsfm_rot_l1l2_residuals (a testing aid): b_e = Log(R_j^T R_ij R_i) by the solve's edge sweep.  Returns dict(b (E x 3), sq, weight)."""
    lib = _abi.load_library()
    n = int(n_cams)
    ei, ej, rel = _rot_l1l2_edges(edge_i, edge_j, rel_aa)
    rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(n, 3)
    E = ei.shape[0]
    b, sq, w = np.empty((E, 3)), np.empty(E), np.empty(E)
    o = _rot_l1l2_options(lib, options)
    st = lib.gsfm_rot_l1l2_residuals(n, E, _p(ei), _p(ej), _p(rel), _p(rot), C.byref(o), _p(b), _p(sq), _p(w))
    _raise_if_failed(lib, "gsfm_rot_l1l2_residuals", st)
    return {"b": b, "sq": sq, "weight": w}


def robust_l1l2_laplacian_solve(n_cams, edge_i, edge_j, rhs, weights=None, fixed_cam=0, **options):
    """gsfm_rot_l1l2_laplacian_solve (a testing aid): x = L_w^-1 rhs on the free cameras by the solve's own structure, product and PCG.
    weights: per edge, None = the unweighted form.  Returns (x (n_cams x 3), dict(cg_iterations, stalled, cg_rel, kernel_ms, product_ms, product_bytes))."""
    lib = _abi.load_library()
    n = int(n_cams)
    ei, ej, _ = _rot_l1l2_edges(edge_i, edge_j, None)
    b = np.ascontiguousarray(rhs, dtype=np.float64).reshape(n, 3)
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != ei.shape[0]:
            raise ValueError("weights disagrees with the edges in length")
    x, info = np.empty((n, 3)), np.zeros(6)
    o = _rot_l1l2_options(lib, options)
    st = lib.gsfm_rot_l1l2_laplacian_solve(n, ei.shape[0], _p(ei), _p(ej), _p(w), int(fixed_cam), _p(b), C.byref(o), _p(x), _p(info))
    _raise_if_failed(lib, "gsfm_rot_l1l2_laplacian_solve", st)
    return x, {"cg_iterations": int(info[0]), "stalled": bool(info[1]), "cg_rel": float(info[2]), "kernel_ms": float(info[3]),
               "product_ms": float(info[4]), "product_bytes": float(info[5])}


def filter_relative_translations(n_cams, edge_i, edge_j, rel_t, rot_aa, num_iterations=48, tolerance=0.1, seed=1, axes=None,
                                 want_projections=False):
    """gsfm_pos_filter_relative_translations: the 1DSfM filter of relative translations (Theia's FilterViewPairsFromRelativeTranslation
    under the reproducible definition of include/gsfm_pos.h) on the device.  rel_t: E x 3 position_2 of each view pair; rot_aa: N x 3
    orientations; axes: num_iterations x 3 projection axes, None = drawn by the library from `seed` (not the reference's axes).
    Returns (keep mask, dict(bad_weight, n_kept, mean, variance, axes, projections (E x num_iterations, or None), num_passes, num_picks
    (per projection), kernel_ms))."""
    lib = _abi.load_library()
    n, K = int(n_cams), int(num_iterations)
    ei = np.ascontiguousarray(edge_i, dtype=np.uint32).reshape(-1)
    ej = np.ascontiguousarray(edge_j, dtype=np.uint32).reshape(-1)
    rel = np.ascontiguousarray(rel_t, dtype=np.float64).reshape(-1, 3)
    rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(n, 3)
    E = ei.shape[0]
    if ej.shape[0] != E or rel.shape[0] != E:
        raise ValueError("edge_i, edge_j and rel_t must describe the same edges")
    ax = None
    if axes is not None:
        ax = np.ascontiguousarray(axes, dtype=np.float64).reshape(-1, 3)
        if ax.shape[0] != K:
            raise ValueError("axes must hold num_iterations rows")
    Kc = max(K, 0)
    bad, keep = np.empty(E), np.empty(E, dtype=np.uint8)
    stats, axes_out = np.empty(6), np.empty((Kc, 3))
    proj = np.empty((E, Kc)) if want_projections else None
    passes, picks = np.zeros(Kc, dtype=np.uint32), np.zeros(Kc, dtype=np.uint32)
    kept, ms = C.c_uint64(0), C.c_double(0)
    st = lib.gsfm_pos_filter_relative_translations(n, E, _p(ei), _p(ej), _p(rel), _p(rot), K, _p(ax), int(seed), float(tolerance),
                                                   _p(bad), _p(keep), C.byref(kept), _p(stats), _p(axes_out),
                                                   _p(proj), _p(passes), _p(picks), C.byref(ms))
    _raise_if_failed(lib, "gsfm_pos_filter_relative_translations", st)
    return keep.astype(bool), {"bad_weight": bad, "n_kept": int(kept.value), "mean": stats[:3].copy(), "variance": stats[3:].copy(), "axes": axes_out,
                               "projections": proj, "num_passes": passes, "num_picks": picks, "kernel_ms": ms.value}


def refine_relative_translations(n_cams, edge_i, edge_j, match_ptr, matches, intrinsics, rot_aa, rel_t):
    """gsfm_pos_refine_relative_translations: every view pair's relative translation refined with the known rotations (Theia's
    OptimizeRelativePositionWithKnownRotation under the definition of include/gsfm_pos.h) on the device, one wavefront per edge.
    match_ptr: E + 1 offsets into matches (rows of x1 y1 x2 y2 in pixels); intrinsics: E x 6 (f1 u1 v1 f2 u2 v2); rot_aa: N x 3
    orientations; rel_t: E x 3 position_2 of each pair (returned for skipped and non-finite edges).
    Returns (rel_t_out E x 3, dict(status (0 refined, 1 skipped, 2 non-finite), iterations, cost, kernel_ms))."""
    lib = _abi.load_library()
    n = int(n_cams)
    ei = np.ascontiguousarray(edge_i, dtype=np.uint32).reshape(-1)
    ej = np.ascontiguousarray(edge_j, dtype=np.uint32).reshape(-1)
    mp = np.ascontiguousarray(match_ptr, dtype=np.uint64).reshape(-1)
    E = ei.shape[0]
    m = np.ascontiguousarray(matches, dtype=np.float64).reshape(-1, 4)
    K = np.ascontiguousarray(intrinsics, dtype=np.float64).reshape(E, 6)
    rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(n, 3)
    rel = np.ascontiguousarray(rel_t, dtype=np.float64).reshape(-1, 3)
    if ej.shape[0] != E or rel.shape[0] != E or mp.shape[0] != E + 1:
        raise ValueError("edge_i, edge_j, rel_t, intrinsics and match_ptr must describe the same edges")
    if E and int(mp.max()) > m.shape[0]:
        raise ValueError("match_ptr points past the end of matches")
    out = np.empty((E, 3))
    status, iters = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
    cost = np.zeros(E)
    ms = C.c_double(0)
    st = lib.gsfm_pos_refine_relative_translations(n, E, _p(ei), _p(ej), _p(mp), _p(m), _p(K), _p(rot), _p(rel), _p(out), _p(status), _p(iters), _p(cost),
                                                   C.byref(ms))
    _raise_if_failed(lib, "gsfm_pos_refine_relative_translations", st)
    return out, {"status": status, "iterations": iters, "cost": cost, "kernel_ms": ms.value}


def _track_arrays(cameras, track_ptr, obs_cam, obs_xy, cam_estimated=None, point_estimated=None, points=None, per=("camera", "track")):
    """What every entry over cameras and a track CSR takes, as contiguous arrays with the shapes checked.  cameras: (name, N x 3 array) pairs
    that must agree in N; points: T x 3 or None; per: the nouns in the messages of the flag arrays.
    Returns (camera arrays, track_ptr, obs_cam, obs_xy, camera flags or None, point flags or None, points or None)."""
    cams = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3) for _, a in cameras]
    tp = np.ascontiguousarray(track_ptr, dtype=np.uint64).reshape(-1)
    oc = np.ascontiguousarray(obs_cam, dtype=np.uint32).reshape(-1)
    xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
    pts = None if points is None else np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    if any(c.shape[0] != cams[0].shape[0] for c in cams):
        names = [name for name, _ in cameras]
        raise ValueError("%s and %s must describe the same cameras" % (", ".join(names[:-1]), names[-1]))
    if tp.shape[0] < 1 or xy.shape[0] != oc.shape[0]:
        raise ValueError("track_ptr needs n_tracks + 1 entries, and obs_cam and obs_xy one row per observation")
    if int(tp.max()) > oc.shape[0]:
        raise ValueError("track_ptr points past the end of the observations")
    T = tp.shape[0] - 1
    if pts is not None and pts.shape[0] != T:
        raise ValueError("points needs one row per track")

    def flags(a, count, what, noun):
        if a is None:
            return None
        a = np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8).reshape(-1)
        if a.shape[0] != count:
            raise ValueError("%s needs one flag per %s" % (what, noun))
        return a
    return cams, tp, oc, xy, flags(cam_estimated, cams[0].shape[0], "cam_estimated", per[0]), flags(point_estimated, T, "point_estimated", per[1]), pts


def triangulate_tracks(rot_aa, cam_pos, intrinsics, track_ptr, obs_cam, obs_xy, cam_estimated=None, min_triangulation_angle_degrees=4.0,
                       max_reprojection_error_pixels=15.0, refine=False, loss=None, max_num_iterations=100, **refine_options):
    """gsfm_tracks_triangulate: every track triangulated by the midpoint method and gated on triangulation angle and reprojection error
    (Theia's TrackEstimator::EstimateTrack without the per-track refinement, under the definition of include/gsfm_tracks.h) on the device,
    a group of 4, 16 or 64 lanes per track.  rot_aa, cam_pos: N x 3; intrinsics: N x 3 (f u v); track_ptr: T + 1 offsets into obs_cam
    (camera index) and obs_xy (pixels); cam_estimated: N flags or None (all estimated).  The defaults are the reference pipeline's.
    Returns dict(points T x 3, status (0 estimated, 1 too few views, 2 angle, 3 Cholesky, 4 behind a camera, 5 reprojection error),
    n_views, mean_sq_err, counts (6), kernel_ms).
    refine=True: gsfm_tracks_triangulate_refine -- between the midpoint and the gate every track's point is refined by Levenberg-Marquardt
    with the cameras held (Theia's BundleAdjustTrack).  loss: None (Ceres' NULL loss), a list of (kind, p0, p1, p2) nodes or an object with
    .native_program(); one Trivial / Huber / SoftLOne / Tukey / GemanMcClure leaf.  The dict then also holds iterations, initial_cost,
    final_cost, termination (per track, -1 = not refined), counts has 7 entries and status 6 is "refinement failed".  refine_options: further
    fields of gsfm_tracks_refine_options by name (function_tolerance, parameter_tolerance, ...)."""
    lib = _abi.load_library()
    if refine_options and not refine:
        raise TypeError("refinement options without refine=True: %s" % sorted(refine_options))
    (rot, pos, K), tp, oc, xy, est, _, _ = _track_arrays((("rot_aa", rot_aa), ("cam_pos", cam_pos), ("intrinsics", intrinsics)), track_ptr, obs_cam, obs_xy,
                                                         cam_estimated)
    T = tp.shape[0] - 1
    points, status, n_views, err = np.zeros((T, 3)), np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32), np.zeros(T)
    counts, ms = np.zeros(7 if refine else 6, dtype=np.uint64), C.c_double(0)
    scene = (rot.shape[0], _p(rot), _p(pos), _p(K), _p(est), T, _p(tp), _p(oc), _p(xy), float(min_triangulation_angle_degrees),
             float(max_reprojection_error_pixels))
    out = (_p(points), _p(status), _p(n_views), _p(err))
    more = {}
    if refine:
        prog, n_nodes = _abi.make_program(_loss_nodes(loss, "track refinement"))
        opt = _abi.TrackRefineOptions()
        lib.gsfm_tracks_refine_default_options(C.byref(opt))
        opt.refine, opt.max_num_iterations = 1, int(max_num_iterations)
        for name, value in refine_options.items():
            if name not in [f for f, _ in _abi.TrackRefineOptions._fields_]:
                raise TypeError("gsfm_tracks_refine_options has no field %r" % name)
            setattr(opt, name, value)
        iters, term, cost0, cost1 = np.zeros(T, dtype=np.int32), np.full(T, -1, dtype=np.int32), np.zeros(T), np.zeros(T)
        st = lib.gsfm_tracks_triangulate_refine(*scene, C.byref(opt), prog, n_nodes, *out, _p(iters), _p(cost0), _p(cost1), _p(term), _p(counts), C.byref(ms))
        _raise_if_failed(lib, "gsfm_tracks_triangulate_refine", st)
        more = {"iterations": iters, "initial_cost": cost0, "final_cost": cost1, "termination": term}
    else:
        _raise_if_failed(lib, "gsfm_tracks_triangulate", lib.gsfm_tracks_triangulate(*scene, *out, _p(counts), C.byref(ms)))
    return dict({"points": points, "status": status, "n_views": n_views, "mean_sq_err": err, "counts": counts, "kernel_ms": ms.value}, **more)


def outlier_tracks(rot_aa, cam_pos, intrinsics, track_ptr, obs_cam, obs_xy, points, cam_estimated=None, point_estimated=None,
                   max_reprojection_error_pixels=5.0, min_triangulation_angle_degrees=4.0):
    """gsfm_tracks_outlier_tracks: the outlier rule after a bundle adjustment (Theia's SetOutlierTracksToUnestimated under the definition of
    include/gsfm_tracks.h) on the device, a group of 4, 16 or 64 lanes per estimated track.  The cameras and tracks of triangulate_tracks;
    points: T x 3; point_estimated: T flags or None (all estimated).  The defaults are Theia's.  Nothing is modified: the caller drops the
    tracks of the statuses 2 to 4.
    Returns dict(status (0 kept, 1 not estimated on input, 2 behind a camera, 3 reprojection error, 4 insufficient viewing angle), n_views,
    mean_sq_err, counts (5), kernel_ms)."""
    lib = _abi.load_library()
    (rot, pos, K), tp, oc, xy, est, pest, pts = _track_arrays((("rot_aa", rot_aa), ("cam_pos", cam_pos), ("intrinsics", intrinsics)), track_ptr, obs_cam,
                                                              obs_xy, cam_estimated, point_estimated, points=points)
    T = tp.shape[0] - 1
    status, n_views = np.zeros(T, dtype=np.int32), np.zeros(T, dtype=np.int32)
    err, counts = np.zeros(T), np.zeros(5, dtype=np.uint64)
    ms = C.c_double(0)
    st = lib.gsfm_tracks_outlier_tracks(rot.shape[0], _p(rot), _p(pos), _p(K), _p(est), T, _p(tp), _p(oc), _p(xy), _p(pts), _p(pest),
                                        float(max_reprojection_error_pixels), float(min_triangulation_angle_degrees), _p(status), _p(n_views), _p(err),
                                        _p(counts), C.byref(ms))
    _raise_if_failed(lib, "gsfm_tracks_outlier_tracks", st)
    return {"status": status, "n_views": n_views, "mean_sq_err": err, "counts": counts, "kernel_ms": ms.value}


TRACK_SELECT_COUNTS = ("tracks_with_items", "cells", "selected_by_cell", "cameras_topped_up", "selected_by_top_up", "selected")


def select_good_tracks(rot_aa, cam_pos, intrinsics, track_ptr, obs_cam, obs_xy, points, cam_estimated=None, point_estimated=None,
                       long_track_length_threshold=10, image_grid_cell_size_pixels=100, min_num_optimized_tracks_per_view=200, hash_capacity_log2=0):
    """gsfm_tracks_select_good: the tracks a bundle adjustment is given (Theia's SelectGoodTracksForBundleAdjustment under the definition of
    include/gsfm_tracks.h) on the device: per camera and grid cell the track with the smallest (min(length, threshold), mean squared
    reprojection error), then every camera topped up to min_num_optimized_tracks_per_view tracks by ascending track index.  The cameras,
    tracks, points and flags of outlier_tracks; the defaults are Theia's.  hash_capacity_log2: the cell table's size, 0 = automatic (a
    test's handle on the probe chains).  Nothing is modified: the caller hands `selected != 0` (and its own flags) to a bundle solver.
    Returns dict(selected (uint8: 0, 1 by a cell, 2 by the top-up), n_views, mean_sq_err, counts (dict of TRACK_SELECT_COUNTS), kernel_ms,
    deficient_items (what the host downloaded for the top-up), replay_ms (the host's walk over them))."""
    lib = _abi.load_library()
    (rot, pos, K), tp, oc, xy, est, pest, pts = _track_arrays((("rot_aa", rot_aa), ("cam_pos", cam_pos), ("intrinsics", intrinsics)), track_ptr, obs_cam,
                                                              obs_xy, cam_estimated, point_estimated, points=points)
    T = tp.shape[0] - 1
    selected, n_views, err = np.zeros(T, dtype=np.uint8), np.zeros(T, dtype=np.int32), np.zeros(T)
    counts, ms, top_up = np.zeros(6, dtype=np.uint64), C.c_double(0), np.zeros(2)
    st = lib.gsfm_tracks_select_good(rot.shape[0], _p(rot), _p(pos), _p(K), _p(est), T, _p(tp), _p(oc), _p(xy), _p(pts), _p(pest),
                                     int(long_track_length_threshold), int(image_grid_cell_size_pixels), int(min_num_optimized_tracks_per_view),
                                     int(hash_capacity_log2), _p(selected), _p(n_views), _p(err), _p(counts), C.byref(ms), _p(top_up))
    _raise_if_failed(lib, "gsfm_tracks_select_good", st)
    return {"selected": selected, "n_views": n_views, "mean_sq_err": err, "counts": {k: int(v) for k, v in zip(TRACK_SELECT_COUNTS, counts)},
            "kernel_ms": ms.value, "deficient_items": int(top_up[0]), "replay_ms": float(top_up[1])}


def select_good_tracks_from_statistics(n_cams, track_ptr, obs_cam, obs_xy, n_views, mean_sq_err, cam_estimated=None, point_estimated=None,
                                       long_track_length_threshold=10, image_grid_cell_size_pixels=100, min_num_optimized_tracks_per_view=200):
    """gsfm_tracks_select_good_from_statistics: the grid cells and the top-up of select_good_tracks as sequential host code (no device), given
    n_views and mean_sq_err per track.  Returns dict(selected, counts (dict of TRACK_SELECT_COUNTS))."""
    lib = _abi.load_library()
    _, tp, oc, xy, est, pest, _ = _track_arrays((("cameras", np.zeros((int(n_cams), 3))),), track_ptr, obs_cam, obs_xy, cam_estimated, point_estimated)
    T = tp.shape[0] - 1
    nv = np.ascontiguousarray(n_views, dtype=np.int32).reshape(-1)
    err = np.ascontiguousarray(mean_sq_err, dtype=np.float64).reshape(-1)
    if nv.shape[0] != T or err.shape[0] != T:
        raise ValueError("n_views and mean_sq_err need one entry per track")
    selected, counts = np.zeros(T, dtype=np.uint8), np.zeros(6, dtype=np.uint64)
    st = lib.gsfm_tracks_select_good_from_statistics(int(n_cams), _p(est), T, _p(tp), _p(oc), _p(xy), _p(pest), _p(nv), _p(err),
                                                     int(long_track_length_threshold), int(image_grid_cell_size_pixels),
                                                     int(min_num_optimized_tracks_per_view), _p(selected), _p(counts))
    _raise_if_failed(lib, "gsfm_tracks_select_good_from_statistics", st)
    return {"selected": selected, "counts": {k: int(v) for k, v in zip(TRACK_SELECT_COUNTS, counts)}}


def track_launch_order(track_ptr):
    """gsfm_tracks_launch_order (host code): (order, class_begin) -- the tracks by lane class 4, 16, 64, longest first inside a class."""
    lib = _abi.load_library()
    tp = np.ascontiguousarray(track_ptr, dtype=np.uint64).reshape(-1)   # (no observations here: _track_arrays does not fit)
    T = tp.shape[0] - 1
    order, begin = np.zeros(T, dtype=np.uint32), np.zeros(4, dtype=np.uint64)
    st = lib.gsfm_tracks_launch_order(T, _p(tp), _p(order), _p(begin))
    _raise_if_failed(lib, "gsfm_tracks_launch_order", st)
    return order, begin


TRACK_BUILD_COUNTS = ("features", "components", "small", "inconsistent", "degenerate", "replayed", "tracks")


def build_tracks(n_views, edge_i, edge_j, match_ptr, matches, min_track_length=2, max_track_length=1000, hash_capacity_log2=0, sequential=False):
    """gsfm_tracks_build: tracks from two-view matches (Theia's TrackBuilder under the definition of include/gsfm_tracks.h) on the device.
    edge_i, edge_j: the E view pairs; match_ptr: E + 1 offsets into matches (rows of x1 y1 x2 y2 in pixels, in the order of Theia's
    AddFeatureCorrespondence calls).  hash_capacity_log2: the feature table's size, 0 = automatic (a test's handle on the probe chains).
    sequential=True: gsfm_tracks_build_sequential, the same definition as sequential host code (no device).
    Returns dict(track_ptr T + 1, obs_view, obs_xy O x 2, counts (dict of TRACK_BUILD_COUNTS), kernel_ms)."""
    lib = _abi.load_library()
    ei = np.ascontiguousarray(edge_i, dtype=np.uint32).reshape(-1)
    ej = np.ascontiguousarray(edge_j, dtype=np.uint32).reshape(-1)
    mp = np.ascontiguousarray(match_ptr, dtype=np.uint64).reshape(-1)
    m = np.ascontiguousarray(matches, dtype=np.float64).reshape(-1, 4)
    E = ei.shape[0]
    if ej.shape[0] != E or mp.shape[0] != E + 1:
        raise ValueError("edge_i, edge_j and match_ptr must describe the same edges")
    if int(mp.max()) > m.shape[0]:
        raise ValueError("match_ptr points past the end of matches")
    M = int(mp[-1])
    opt = _abi.TrackBuildOptions()
    lib.gsfm_tracks_build_default_options(C.byref(opt))
    opt.min_track_length, opt.max_track_length, opt.hash_capacity_log2 = int(min_track_length), int(max_track_length), int(hash_capacity_log2)
    track_ptr, obs_view, obs_xy = np.zeros(M + 1, dtype=np.uint64), np.zeros(2 * M, dtype=np.uint32), np.zeros((2 * M, 2))
    n_tracks, n_obs, counts, ms = C.c_uint64(0), C.c_uint64(0), np.zeros(7, dtype=np.uint64), C.c_double(0)
    name = "gsfm_tracks_build_sequential" if sequential else "gsfm_tracks_build"
    st = getattr(lib, name)(int(n_views), E, _p(ei), _p(ej), _p(mp), _p(m), C.byref(opt), _p(track_ptr), _p(obs_view), _p(obs_xy), C.byref(n_tracks),
                            C.byref(n_obs), _p(counts), C.byref(ms))
    _raise_if_failed(lib, name, st)
    T, O = int(n_tracks.value), int(n_obs.value)
    return {"track_ptr": track_ptr[:T + 1].copy(), "obs_view": obs_view[:O].copy(), "obs_xy": obs_xy[:O].copy(),
            "counts": {k: int(v) for k, v in zip(TRACK_BUILD_COUNTS, counts)}, "kernel_ms": ms.value}


class PositionProblem(ProblemBase):
    """Camera positions from relative translations (include/gsfm_pos.h): the reference's EstimatePositions with BASELINE residuals
    r = (c_j - c_i) / |c_j - c_i| - R(aa_i)^T t_ij on the device.  rel_t: E x 3 position_2 of each view pair (frame of camera i);
    rot_aa: N x 3 angle-axis orientations.  A new problem has Ceres' NULL loss; set_loss takes the rotation path's descriptors."""

    _prefix = "gsfm_pos_"

    def __init__(self, n_cams, edge_i, edge_j, rel_t, rot_aa):
        lib = _abi.load_library()
        ei = np.ascontiguousarray(edge_i, dtype=np.uint32)
        ej = np.ascontiguousarray(edge_j, dtype=np.uint32)
        rel = np.ascontiguousarray(rel_t, dtype=np.float64).reshape(-1, 3)
        rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(int(n_cams), 3)
        if not (ei.shape == ej.shape == (rel.shape[0],)):
            raise ValueError("edge_i, edge_j and rel_t must describe the same edges")
        h = C.c_void_p()
        st = lib.gsfm_pos_problem_create(int(n_cams), ei.size, _p(ei), _p(ej), _p(rel), _p(rot), C.byref(h))
        _raise_if_failed(lib, "gsfm_pos_problem_create", st)
        ProblemBase.__init__(self, lib, h, n_cams, ei.size, -1, 3)

    def _last_error(self):
        return self._lib.gsfm_last_error().decode("utf-8", "replace")

    def default_options(self):
        o = _abi.PosOptions()
        self._lib.gsfm_pos_options_default(C.byref(o))
        return o

    def solve(self, init=None, fixed_cam=0, **options):
        """init: N x 3 start positions, None = the reference's all-zero start.  fixed_cam: the camera held constant (-1: none).
        Returns (positions, summary dict)."""
        pos = np.zeros((self.n_cams, 3)) if init is None else np.array(init, dtype=np.float64, order="C").reshape(self.n_cams, 3)
        o = self._options(options)
        s = _abi.PosSummary()
        st = self._lib.gsfm_pos_solve(self._h, _p(pos), int(fixed_cam), C.byref(o), C.byref(s))
        self._check(st, "solve")
        return pos, s.as_dict()

    def residuals(self, pos):
        """(r: E x 3, rho: E) at pos"""
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(self.n_cams, 3)
        r = np.empty((self.n_edges, 3))
        rho = np.empty(self.n_edges)
        st = self._lib.gsfm_pos_residuals(self._h, _p(pos), _p(r), _p(rho))
        self._check(st, "residuals")
        return r, rho

    # linearize(pos) and normal_matvec(v) are ProblemBase's: gsfm_pos_linearize / gsfm_pos_normal_matvec share gsfm_rot_'s argument lists

    def step_check(self, pos, fixed_cam=0, radius=1e4, want_K=True, **options):
        """gsfm_pos_step_check: one LM step's linear algebra at pos (iteration 1 of a solve from pos, at `radius`).  Returns a dict:
        K (3N x 3N, when the dense path assembled it, else None), b, y, delta (N x 3), model_cost_change, dg, dld, cg_rel, path (0 dense, 1 PCG),
        chol_info, cg_iterations."""
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(self.n_cams, 3)
        o = self._options(options)
        n = 3 * self.n_cams
        K = np.full((n, n), np.nan) if want_K else None
        b, y, delta = np.empty((self.n_cams, 3)), np.empty((self.n_cams, 3)), np.empty((self.n_cams, 3))
        scal = np.empty(4)
        info = np.zeros(3, dtype=np.int32)
        st = self._lib.gsfm_pos_step_check(self._h, _p(pos), int(fixed_cam), float(radius), C.byref(o), None if K is None else _p(K),
                                           _p(b), _p(y), _p(delta), _p(scal), _p(info))
        self._check(st, "step_check")
        return {"K": K if info[1] >= 0 else None, "b": b, "y": y, "delta": delta,
                "model_cost_change": scal[0], "dg": scal[1], "dld": scal[2], "cg_rel": scal[3], "path": int(info[0]),
                "chol_info": int(info[1]), "cg_iterations": int(info[2])}

    def set_edge_weights(self, w):
        raise NotImplementedError("position residuals have weight 1 (the reference's BASELINE error)")


_PER_ENTRY = ("entry", "entry")   # the bundle classes' wording for both flag arrays


class _BundleProblemBase(_Handle):
    """What BundleProblem and FullBundleProblem share: the handle, the loss, the options, the argument arrays.  A subclass sets _prefix (the
    C prefix of its entry points), creates the problem in __init__ and ends it with self._adopt(lib, handle, n_cams, n_tracks, n_obs)."""
    def _adopt(self, lib, handle, n_cams, n_tracks, n_obs):
        self._lib, self._h = lib, handle
        self.n_cams, self.n_tracks, self.n_obs = n_cams, n_tracks, n_obs

    def _check(self, st, what):
        if st != 0:
            raise SolverError("%s failed with status %d: %s" % (what, st, self._lib.gsfm_last_error().decode("utf-8", "replace")))

    def set_loss(self, loss):
        """loss: None (Ceres' NULL loss), a list of (kind, p0, p1, p2) nodes or an object with .native_program(); one Trivial / Huber /
        SoftLOne / Tukey / GemanMcClure leaf."""
        arr, n = _abi.make_program(_loss_nodes(loss, "bundle adjustment"))
        self._check(self._fn("set_loss")(self._h, arr, n), "set_loss")

    def default_options(self):
        o = _abi.BaOptions()
        self._fn("options_default")(C.byref(o))
        return o

    def _point(self, cam_pos, points):
        return (np.array(cam_pos, dtype=np.float64, order="C").reshape(self.n_cams, 3),
                np.array(points, dtype=np.float64, order="C").reshape(self.n_tracks, 3))


class BundleProblem(_BundleProblemBase):
    """Bundle adjustment of camera positions and points with fixed orientations (include/gsfm_ba.h): Theia's
    BundleAdjustCameraPositionsAndPoints on the device, the points eliminated and the reduced camera system solved by PCG.
    rot_aa: N x 3, intrinsics: N x 3 (f u v); track_ptr / obs_cam / obs_xy: the track CSR of triangulate_tracks; cam_estimated (N) and
    point_estimated (T): flags or None (all estimated).  A new problem has Ceres' NULL loss."""
    _prefix = "gsfm_ba_"

    def __init__(self, rot_aa, intrinsics, track_ptr, obs_cam, obs_xy, cam_estimated=None, point_estimated=None):
        lib = _abi.load_library()
        rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(-1, 3)
        (K,), tp, oc, xy, ce, pe, _ = _track_arrays((("intrinsics", intrinsics),), track_ptr, obs_cam, obs_xy, cam_estimated, point_estimated, per=_PER_ENTRY)
        n, T = rot.shape[0], tp.shape[0] - 1
        if K.shape[0] != n:   # (after the track arrays, as ever)
            raise ValueError("rot_aa and intrinsics must describe the same cameras")
        h = C.c_void_p()
        st = lib.gsfm_ba_problem_create(n, _p(rot), _p(K), _p(ce), T, _p(tp), _p(oc), _p(xy), _p(pe), C.byref(h))
        _raise_if_failed(lib, "gsfm_ba_problem_create", st)
        self._adopt(lib, h, n, T, int(oc.shape[0]))

    def solve(self, cam_pos, points, **options):
        """Returns (camera positions N x 3, points T x 3, summary dict); inactive and unestimated rows are returned as given."""
        c, p = self._point(cam_pos, points)
        o, s = self._options(options), _abi.BaSummary()
        self._check(self._lib.gsfm_ba_solve(self._h, _p(c), _p(p), C.byref(o), C.byref(s)), "solve")
        return c, p, s.as_dict()

    def residuals(self, cam_pos, points):
        """(r: n_obs x 2, rho: n_obs); zeros for an unused observation"""
        c, p = self._point(cam_pos, points)
        r, rho = np.zeros((self.n_obs, 2)), np.zeros(self.n_obs)
        self._check(self._lib.gsfm_ba_residuals(self._h, _p(c), _p(p), _p(r), _p(rho)), "residuals")
        return r, rho

    def linearize(self, cam_pos, points):
        """dict(cost, grad_cam N x 3, grad_point T x 3, diag_cam N x 3 x 3, diag_point T x 3 x 3)"""
        c, p = self._point(cam_pos, points)
        cost = np.zeros(1)
        gc, gp = np.zeros((self.n_cams, 3)), np.zeros((self.n_tracks, 3))
        dc, dp = np.zeros((self.n_cams, 3, 3)), np.zeros((self.n_tracks, 3, 3))
        self._check(self._lib.gsfm_ba_linearize(self._h, _p(c), _p(p), _p(cost), _p(gc), _p(gp), _p(dc), _p(dp)), "linearize")
        return {"cost": float(cost[0]), "grad_cam": gc, "grad_point": gp, "diag_cam": dc, "diag_point": dp}

    def schur_matvec(self, v, radius=1e4, **options):
        """y = Sc v (N x 3) for the last linearize / step_check, damped at `radius`"""
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(self.n_cams, 3)
        y = np.zeros((self.n_cams, 3))
        o = self._options(options)
        self._check(self._lib.gsfm_ba_schur_matvec(self._h, _p(v), float(radius), C.byref(o), _p(y)), "schur_matvec")
        return y

    def step_check(self, cam_pos, points, radius=1e4, **options):
        """gsfm_ba_step_check: dict(rhs, y_cam, y_point, delta_cam, delta_point, model_cost_change, dg, dld, cg_rel, cg_iterations, stalled)"""
        c, p = self._point(cam_pos, points)
        o = self._options(options)
        N, T = self.n_cams, self.n_tracks
        rhs, yc, yp, dc, dp = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((T, 3)), np.zeros((N, 3)), np.zeros((T, 3))
        scal, info = np.zeros(4), np.zeros(2, dtype=np.int32)
        st = self._lib.gsfm_ba_step_check(self._h, _p(c), _p(p), float(radius), C.byref(o), _p(rhs), _p(yc), _p(yp), _p(dc), _p(dp), _p(scal),
                                          _p(info))
        self._check(st, "step_check")
        return {"rhs": rhs, "y_cam": yc, "y_point": yp, "delta_cam": dc, "delta_point": dp, "model_cost_change": scal[0], "dg": scal[1],
                "dld": scal[2], "cg_rel": scal[3], "cg_iterations": int(info[0]), "stalled": bool(info[1])}


    def time_kernels(self, cam_pos, points, radius=1e4, reps=10):
        """mean device microseconds of the kernels of one linearisation and one Schur product (gsfm_ba_time_kernels)"""
        c, p = self._point(cam_pos, points)
        out = np.zeros(6)
        self._check(self._lib.gsfm_ba_time_kernels(self._h, _p(c), _p(p), float(radius), int(reps), _p(out)), "time_kernels")
        return dict(zip(("lin_tracks", "lin_cameras", "cost", "point_pass", "camera_pass", "preconditioner"), out))


def bundle_adjust_positions_and_points(rot_aa, cam_pos, intrinsics, track_ptr, obs_cam, obs_xy, points, cam_estimated=None, point_estimated=None,
                                       loss=None, **options):
    """One call: BundleProblem(...).set_loss(loss).solve(cam_pos, points, **options).  Returns (cam_pos, points, summary dict)."""
    prob = BundleProblem(rot_aa, intrinsics, track_ptr, obs_cam, obs_xy, cam_estimated, point_estimated)
    try:
        prob.set_loss(loss)
        return prob.solve(cam_pos, points, **options)
    finally:
        prob.close()


class PointPositionProblem(_BundleProblemBase):
    """Camera positions from relative translations AND feature tracks (include/gsfm_posp.h): PositionProblem's edges plus, per track, one
    point tied to every camera that sees it by the direction residual w_p ((X - c) / |X - c| - ray); the points are eliminated and the
    reduced camera system is solved by PCG.  edge_i / edge_j / rel_t / rot_aa: as PositionProblem; ray_rot_aa: N x 3 orientations the
    feature rays are rotated by (None: rot_aa); intrinsics: N x 3 (f u v); track_ptr / obs_cam / obs_xy: the track CSR of triangulate_tracks
    (track_ptr None: no tracks).  A new problem has Ceres' NULL loss; set_loss takes PositionProblem's native losses."""
    _prefix = "gsfm_posp_"

    def __init__(self, n_cams, edge_i, edge_j, rel_t, rot_aa, ray_rot_aa=None, intrinsics=None, track_ptr=None, obs_cam=None, obs_xy=None,
                 point_to_camera_weight=0.5):
        lib = _abi.load_library()
        n = int(n_cams)
        ei = np.ascontiguousarray(edge_i, dtype=np.uint32)
        ej = np.ascontiguousarray(edge_j, dtype=np.uint32)
        rel = np.ascontiguousarray(rel_t, dtype=np.float64).reshape(-1, 3)
        rot = np.ascontiguousarray(rot_aa, dtype=np.float64).reshape(n, 3)
        if not (ei.shape == ej.shape == (rel.shape[0],)):
            raise ValueError("edge_i, edge_j and rel_t must describe the same edges")
        if track_ptr is None:
            track_ptr, obs_cam, obs_xy = np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros((0, 2))
        ray = rot if ray_rot_aa is None else ray_rot_aa
        K = np.zeros((n, 3)) if intrinsics is None else intrinsics
        (ray, K), tp, oc, xy, _, _, _ = _track_arrays((("ray_rot_aa", ray), ("intrinsics", K)), track_ptr, obs_cam, obs_xy, per=_PER_ENTRY)
        if ray.shape[0] != n:
            raise ValueError("rot_aa, ray_rot_aa and intrinsics must describe the same cameras")
        T = tp.shape[0] - 1
        h = C.c_void_p()
        st = lib.gsfm_posp_problem_create(n, ei.size, _p(ei), _p(ej), _p(rel), _p(rot), _p(ray), _p(K), T, _p(tp), _p(oc), _p(xy),
                                          float(point_to_camera_weight), C.byref(h))
        _raise_if_failed(lib, "gsfm_posp_problem_create", st)
        self._adopt(lib, h, n, T, int(oc.shape[0]))
        self.n_edges = int(ei.size)

    def set_loss(self, loss):
        """loss: None (Ceres' NULL loss), a list of (kind, p0, p1, p2) nodes or an object with .native_program(), as PositionProblem takes
        them; an object with only .Evaluate (a host callback) is refused by the library."""
        nodes = _loss_nodes(loss, "position problem with points", callback_ok=True)
        if nodes is None:
            self._check(self._lib.gsfm_posp_set_loss_callback(self._h, _abi.LOSS_CALLBACK_FN(), None), "set_loss_callback")
        arr, n = _abi.make_program(nodes)
        self._check(self._lib.gsfm_posp_set_loss(self._h, arr, n), "set_loss")

    def default_options(self):
        o = _abi.PosOptions()
        self._lib.gsfm_pos_options_default(C.byref(o))
        return o

    def _point(self, cam_pos, points):
        c = np.zeros((self.n_cams, 3)) if cam_pos is None else np.array(cam_pos, dtype=np.float64, order="C").reshape(self.n_cams, 3)
        p = np.ones((self.n_tracks, 3)) if points is None else np.array(points, dtype=np.float64, order="C").reshape(self.n_tracks, 3)
        return c, p

    def solve(self, cam_pos=None, points=None, fixed_cam=0, **options):
        """cam_pos / points: start values (None: the reference's, cameras at 0 and points at (1, 1, 1)).  fixed_cam: the camera held constant
        (-1: none).  Returns (camera positions N x 3, points T x 3, summary dict); inactive rows are returned as given."""
        c, p = self._point(cam_pos, points)
        o, s = self._options(options), _abi.PospSummary()
        self._check(self._lib.gsfm_posp_solve(self._h, _p(c), _p(p), int(fixed_cam), C.byref(o), C.byref(s)), "solve")
        return c, p, s.as_dict()

    def residuals(self, cam_pos, points):
        """dict(r_edge E x 3, rho_edge E, r_obs n_obs x 3 (weighted), rho_obs n_obs, ray n_obs x 3); zeros for an observation that is not used"""
        c, p = self._point(cam_pos, points)
        E, O = self.n_edges, self.n_obs
        out = {"r_edge": np.zeros((E, 3)), "rho_edge": np.zeros(E), "r_obs": np.zeros((O, 3)), "rho_obs": np.zeros(O), "ray": np.zeros((O, 3))}
        self._check(self._lib.gsfm_posp_residuals(self._h, _p(c), _p(p), _p(out["r_edge"]), _p(out["rho_edge"]), _p(out["r_obs"]), _p(out["rho_obs"]),
                                                  _p(out["ray"])), "residuals")
        return out

    def linearize(self, cam_pos, points):
        """dict(cost, grad_cam N x 3, grad_point T x 3, diag_cam N x 3 x 3, diag_point T x 3 x 3), every camera of the edges active"""
        c, p = self._point(cam_pos, points)
        cost = np.zeros(1)
        gc, gp = np.zeros((self.n_cams, 3)), np.zeros((self.n_tracks, 3))
        dc, dp = np.zeros((self.n_cams, 3, 3)), np.zeros((self.n_tracks, 3, 3))
        self._check(self._lib.gsfm_posp_linearize(self._h, _p(c), _p(p), _p(cost), _p(gc), _p(gp), _p(dc), _p(dp)), "linearize")
        return {"cost": float(cost[0]), "grad_cam": gc, "grad_point": gp, "diag_cam": dc, "diag_point": dp}

    def schur_matvec(self, v, radius=1e4, **options):
        """y = Sc v (N x 3) for the last linearize / step_check (and its active set), damped at `radius`"""
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(self.n_cams, 3)
        y = np.zeros((self.n_cams, 3))
        o = self._options(options)
        self._check(self._lib.gsfm_posp_schur_matvec(self._h, _p(v), float(radius), C.byref(o), _p(y)), "schur_matvec")
        return y

    def step_check(self, cam_pos, points, fixed_cam=0, radius=1e4, **options):
        """gsfm_posp_step_check: dict(rhs, y_cam, y_point, delta_cam, delta_point, model_cost_change, dg, dld, cg_rel, cg_iterations, stalled)"""
        c, p = self._point(cam_pos, points)
        o = self._options(options)
        N, T = self.n_cams, self.n_tracks
        rhs, yc, yp, dc, dp = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((T, 3)), np.zeros((N, 3)), np.zeros((T, 3))
        scal, info = np.zeros(4), np.zeros(2, dtype=np.int32)
        st = self._lib.gsfm_posp_step_check(self._h, _p(c), _p(p), int(fixed_cam), float(radius), C.byref(o), _p(rhs), _p(yc), _p(yp), _p(dc), _p(dp),
                                            _p(scal), _p(info))
        self._check(st, "step_check")
        return {"rhs": rhs, "y_cam": yc, "y_point": yp, "delta_cam": dc, "delta_point": dp, "model_cost_change": scal[0], "dg": scal[1],
                "dld": scal[2], "cg_rel": scal[3], "cg_iterations": int(info[0]), "stalled": bool(info[1])}

    def time_kernels(self, cam_pos, points, radius=1e4, reps=10):
        """mean device microseconds of the kernels of one linearisation and one Schur product (gsfm_posp_time_kernels)"""
        c, p = self._point(cam_pos, points)
        out = np.zeros(7)
        self._check(self._lib.gsfm_posp_time_kernels(self._h, _p(c), _p(p), float(radius), int(reps), _p(out)), "time_kernels")
        return dict(zip(("rays", "lin_tracks", "lin_cameras", "cost_tracks", "point_pass", "camera_pass", "preconditioner"), out))


def estimate_positions_with_points(n_cams, edge_i, edge_j, rel_t, rot_aa, intrinsics, track_ptr, obs_cam, obs_xy, point_to_camera_weight=0.5,
                                   ray_rot_aa=None, cam_pos=None, points=None, fixed_cam=0, loss=None, **options):
    """One call: PointPositionProblem(...).set_loss(loss).solve(cam_pos, points, fixed_cam, **options).  Returns (cam_pos, points, summary dict)."""
    prob = PointPositionProblem(n_cams, edge_i, edge_j, rel_t, rot_aa, ray_rot_aa, intrinsics, track_ptr, obs_cam, obs_xy, point_to_camera_weight)
    try:
        prob.set_loss(loss)
        return prob.solve(cam_pos, points, fixed_cam, **options)
    finally:
        prob.close()


class FullBundleProblem(_BundleProblemBase):
    """The full bundle adjustment (include/gsfm_ba6.h): Theia's GlobalReconstructionEstimator::BundleAdjustment on the device, camera
    orientations, camera positions and points moving together (intrinsics held), the points eliminated and the reduced 6 x 6-block camera
    system solved by PCG.  The arguments are BundleProblem's without rot_aa: the orientations are a start value of solve()."""
    _prefix = "gsfm_ba6_"

    def __init__(self, intrinsics, track_ptr, obs_cam, obs_xy, cam_estimated=None, point_estimated=None):
        lib = _abi.load_library()
        (K,), tp, oc, xy, ce, pe, _ = _track_arrays((("intrinsics", intrinsics),), track_ptr, obs_cam, obs_xy, cam_estimated, point_estimated, per=_PER_ENTRY)
        n, T = K.shape[0], tp.shape[0] - 1
        h = C.c_void_p()
        st = lib.gsfm_ba6_problem_create(n, _p(K), _p(ce), T, _p(tp), _p(oc), _p(xy), _p(pe), C.byref(h))
        _raise_if_failed(lib, "gsfm_ba6_problem_create", st)
        self._adopt(lib, h, n, T, int(oc.shape[0]))

    def _point6(self, rot_aa, cam_pos, points):
        return (np.array(rot_aa, dtype=np.float64, order="C").reshape(self.n_cams, 3), ) + self._point(cam_pos, points)

    def solve(self, rot_aa, cam_pos, points, **options):
        """Returns (orientations N x 3, camera positions N x 3, points T x 3, summary dict); inactive and unestimated rows are returned as given."""
        w, c, p = self._point6(rot_aa, cam_pos, points)
        o, s = self._options(options), _abi.BaSummary()
        self._check(self._lib.gsfm_ba6_solve(self._h, _p(w), _p(c), _p(p), C.byref(o), C.byref(s)), "solve")
        return w, c, p, s.as_dict()

    def residuals(self, rot_aa, cam_pos, points):
        """(r: n_obs x 2, rho: n_obs); zeros for an unused observation"""
        w, c, p = self._point6(rot_aa, cam_pos, points)
        r, rho = np.zeros((self.n_obs, 2)), np.zeros(self.n_obs)
        self._check(self._lib.gsfm_ba6_residuals(self._h, _p(w), _p(c), _p(p), _p(r), _p(rho)), "residuals")
        return r, rho

    def linearize(self, rot_aa, cam_pos, points):
        """dict(cost, grad_rot N x 3, grad_pos N x 3, grad_point T x 3, diag_cam N x 6 x 6 (w then o), diag_point T x 3 x 3)"""
        w, c, p = self._point6(rot_aa, cam_pos, points)
        cost = np.zeros(1)
        gr, gc, gp = np.zeros((self.n_cams, 3)), np.zeros((self.n_cams, 3)), np.zeros((self.n_tracks, 3))
        dc, dp = np.zeros((self.n_cams, 6, 6)), np.zeros((self.n_tracks, 3, 3))
        self._check(self._lib.gsfm_ba6_linearize(self._h, _p(w), _p(c), _p(p), _p(cost), _p(gr), _p(gc), _p(gp), _p(dc), _p(dp)), "linearize")
        return {"cost": float(cost[0]), "grad_rot": gr, "grad_pos": gc, "grad_point": gp, "diag_cam": dc, "diag_point": dp}

    def schur_matvec(self, v, radius=1e4, **options):
        """y = Sc v (N x 6, per camera w then o) for the last linearize / step_check, damped at `radius`"""
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(self.n_cams, 6)
        y = np.zeros((self.n_cams, 6))
        o = self._options(options)
        self._check(self._lib.gsfm_ba6_schur_matvec(self._h, _p(v), float(radius), C.byref(o), _p(y)), "schur_matvec")
        return y

    def step_check(self, rot_aa, cam_pos, points, radius=1e4, **options):
        """gsfm_ba6_step_check: dict(rhs, y_cam (N x 6), y_point, delta_rot, delta_pos, delta_point, j_delta (n_obs x 2), model_cost_change, dg,
        jd2, cg_rel, cg_iterations, stalled)"""
        w, c, p = self._point6(rot_aa, cam_pos, points)
        o = self._options(options)
        N, T = self.n_cams, self.n_tracks
        rhs, yc, yp = np.zeros((N, 6)), np.zeros((N, 6)), np.zeros((T, 3))
        dr, dc, dp, jd = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((T, 3)), np.zeros((self.n_obs, 2))
        scal, info = np.zeros(4), np.zeros(2, dtype=np.int32)
        st = self._lib.gsfm_ba6_step_check(self._h, _p(w), _p(c), _p(p), float(radius), C.byref(o), _p(rhs), _p(yc), _p(yp), _p(dr), _p(dc), _p(dp),
                                           _p(jd), _p(scal), _p(info))
        self._check(st, "step_check")
        return {"rhs": rhs, "y_cam": yc, "y_point": yp, "delta_rot": dr, "delta_pos": dc, "delta_point": dp, "j_delta": jd, "model_cost_change": scal[0],
                "dg": scal[1], "jd2": scal[2], "cg_rel": scal[3], "cg_iterations": int(info[0]), "stalled": bool(info[1])}

    def time_kernels(self, rot_aa, cam_pos, points, radius=1e4, reps=10):
        """mean device microseconds of the kernels of one linearisation and one Schur product (gsfm_ba6_time_kernels)"""
        w, c, p = self._point6(rot_aa, cam_pos, points)
        out = np.zeros(8)
        self._check(self._lib.gsfm_ba6_time_kernels(self._h, _p(w), _p(c), _p(p), float(radius), int(reps), _p(out)), "time_kernels")
        return dict(zip(("camera_records", "lin_tracks", "lin_cameras", "cost", "point_pass", "camera_pass", "preconditioner", "quadratic_form"), out))


def bundle_adjust(rot_aa, cam_pos, intrinsics, track_ptr, obs_cam, obs_xy, points, cam_estimated=None, point_estimated=None, loss=None, **options):
    """One call: FullBundleProblem(...).set_loss(loss).solve(rot_aa, cam_pos, points, **options).  Returns (rot_aa, cam_pos, points, summary dict)."""
    prob = FullBundleProblem(intrinsics, track_ptr, obs_cam, obs_xy, cam_estimated, point_estimated)
    try:
        prob.set_loss(loss)
        return prob.solve(rot_aa, cam_pos, points, **options)
    finally:
        prob.close()


class FocalBundleProblem(_BundleProblemBase):
    """The full bundle adjustment with free focal lengths (include/gsfm_ba7.h): Theia's GlobalReconstructionEstimator::BundleAdjustment with
    intrinsics_to_optimize = FOCAL_LENGTH on the device; a seventh coordinate per camera, the reduced 7 x 7-block camera system solved by PCG.
    The arguments are FullBundleProblem's and focal_free (N flags or None: every camera's focal length is free); column 0 of intrinsics is not
    read: the focal lengths (N, pixels) are a start value of solve().  A camera with focal_free = 0 keeps the focal length given to solve()."""
    _prefix = "gsfm_ba7_"

    def __init__(self, intrinsics, track_ptr, obs_cam, obs_xy, cam_estimated=None, point_estimated=None, focal_free=None):
        lib = _abi.load_library()
        (K,), tp, oc, xy, ce, pe, _ = _track_arrays((("intrinsics", intrinsics),), track_ptr, obs_cam, obs_xy, cam_estimated, point_estimated, per=_PER_ENTRY)
        n, T = K.shape[0], tp.shape[0] - 1
        ff = None
        if focal_free is not None:
            ff = np.ascontiguousarray(np.asarray(focal_free) != 0, dtype=np.uint8).reshape(-1)
            if ff.shape[0] != n:
                raise ValueError("focal_free needs one flag per entry")
        h = C.c_void_p()
        st = lib.gsfm_ba7_problem_create(n, _p(K), _p(ce), _p(ff), T, _p(tp), _p(oc), _p(xy), _p(pe), C.byref(h))
        _raise_if_failed(lib, "gsfm_ba7_problem_create", st)
        self._adopt(lib, h, n, T, int(oc.shape[0]))

    def _point7(self, rot_aa, cam_pos, focal, points):
        c, p = self._point(cam_pos, points)
        return np.array(rot_aa, dtype=np.float64, order="C").reshape(self.n_cams, 3), c, np.array(focal, dtype=np.float64, order="C").reshape(self.n_cams), p

    def solve(self, rot_aa, cam_pos, focal, points, **options):
        """Returns (orientations N x 3, camera positions N x 3, focal lengths N, points T x 3, summary dict); inactive and unestimated rows
        and held focal lengths are returned as given."""
        w, c, f, p = self._point7(rot_aa, cam_pos, focal, points)
        o, s = self._options(options), _abi.BaSummary()
        self._check(self._lib.gsfm_ba7_solve(self._h, _p(w), _p(c), _p(f), _p(p), C.byref(o), C.byref(s)), "solve")
        return w, c, f, p, s.as_dict()

    def residuals(self, rot_aa, cam_pos, focal, points):
        """(r: n_obs x 2, rho: n_obs); zeros for an unused observation"""
        w, c, f, p = self._point7(rot_aa, cam_pos, focal, points)
        r, rho = np.zeros((self.n_obs, 2)), np.zeros(self.n_obs)
        self._check(self._lib.gsfm_ba7_residuals(self._h, _p(w), _p(c), _p(f), _p(p), _p(r), _p(rho)), "residuals")
        return r, rho

    def linearize(self, rot_aa, cam_pos, focal, points):
        """dict(cost, grad_rot N x 3, grad_pos N x 3, grad_focal N, grad_point T x 3, diag_cam N x 7 x 7 (w, o, f), diag_point T x 3 x 3)"""
        w, c, f, p = self._point7(rot_aa, cam_pos, focal, points)
        cost = np.zeros(1)
        gr, gc, gf, gp = np.zeros((self.n_cams, 3)), np.zeros((self.n_cams, 3)), np.zeros(self.n_cams), np.zeros((self.n_tracks, 3))
        dc, dp = np.zeros((self.n_cams, 7, 7)), np.zeros((self.n_tracks, 3, 3))
        st = self._lib.gsfm_ba7_linearize(self._h, _p(w), _p(c), _p(f), _p(p), _p(cost), _p(gr), _p(gc), _p(gf), _p(gp), _p(dc), _p(dp))
        self._check(st, "linearize")
        return {"cost": float(cost[0]), "grad_rot": gr, "grad_pos": gc, "grad_focal": gf, "grad_point": gp, "diag_cam": dc, "diag_point": dp}

    def schur_matvec(self, v, radius=1e4, **options):
        """y = Sc v (N x 7, per camera w, o, f) for the last linearize / step_check, damped at `radius`"""
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(self.n_cams, 7)
        y = np.zeros((self.n_cams, 7))
        o = self._options(options)
        self._check(self._lib.gsfm_ba7_schur_matvec(self._h, _p(v), float(radius), C.byref(o), _p(y)), "schur_matvec")
        return y

    def step_check(self, rot_aa, cam_pos, focal, points, radius=1e4, **options):
        """gsfm_ba7_step_check: dict(rhs, y_cam (N x 7), y_point, delta_rot, delta_pos, delta_focal, delta_point, j_delta (n_obs x 2),
        model_cost_change, dg, jd2, cg_rel, cg_iterations, stalled)"""
        w, c, f, p = self._point7(rot_aa, cam_pos, focal, points)
        o = self._options(options)
        N, T = self.n_cams, self.n_tracks
        rhs, yc, yp = np.zeros((N, 7)), np.zeros((N, 7)), np.zeros((T, 3))
        dr, dc, df, dp, jd = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N), np.zeros((T, 3)), np.zeros((self.n_obs, 2))
        scal, info = np.zeros(4), np.zeros(2, dtype=np.int32)
        st = self._lib.gsfm_ba7_step_check(self._h, _p(w), _p(c), _p(f), _p(p), float(radius), C.byref(o), _p(rhs), _p(yc), _p(yp), _p(dr), _p(dc), _p(df),
                                           _p(dp), _p(jd), _p(scal), _p(info))
        self._check(st, "step_check")
        return {"rhs": rhs, "y_cam": yc, "y_point": yp, "delta_rot": dr, "delta_pos": dc, "delta_focal": df, "delta_point": dp, "j_delta": jd,
                "model_cost_change": scal[0], "dg": scal[1], "jd2": scal[2], "cg_rel": scal[3], "cg_iterations": int(info[0]), "stalled": bool(info[1])}

    def time_kernels(self, rot_aa, cam_pos, focal, points, radius=1e4, reps=10):
        """mean device microseconds of the kernels of one linearisation and one Schur product (gsfm_ba7_time_kernels)"""
        w, c, f, p = self._point7(rot_aa, cam_pos, focal, points)
        out = np.zeros(8)
        self._check(self._lib.gsfm_ba7_time_kernels(self._h, _p(w), _p(c), _p(f), _p(p), float(radius), int(reps), _p(out)), "time_kernels")
        return dict(zip(("camera_records", "lin_tracks", "lin_cameras", "cost", "point_pass", "camera_pass", "preconditioner", "quadratic_form"), out))


def bundle_adjust_focal(rot_aa, cam_pos, focal, intrinsics, track_ptr, obs_cam, obs_xy, points, cam_estimated=None, point_estimated=None, focal_free=None,
                        loss=None, **options):
    """One call: FocalBundleProblem(...).set_loss(loss).solve(rot_aa, cam_pos, focal, points, **options).  Returns (rot_aa, cam_pos, focal,
    points, summary dict)."""
    prob = FocalBundleProblem(intrinsics, track_ptr, obs_cam, obs_xy, cam_estimated, point_estimated, focal_free)
    try:
        prob.set_loss(loss)
        return prob.solve(rot_aa, cam_pos, focal, points, **options)
    finally:
        prob.close()

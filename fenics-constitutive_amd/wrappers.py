"""3D -> plane-strain / uniaxial-strain wrappers (reference: ``models/utils.py:211-412``).

Same contract as the reference classes: a FULL (3-D) model is driven with 1-D / 2-D arrays by
copying the mapped components into cached 3-D arrays, evaluating the 3-D model and copying the
mapped components back; the history is the 3-D model's.  Here the cached 3-D arrays live on
the GPU and the component maps are device kernels (``fcamd_convert_device``), so a 1-D/2-D
problem moves only its own small arrays over PCIe.  Around ``VonMises3D`` the three steps are one
fused kernel (``fcamd_evaluate_device_wrapped``): only the cached 3-D stress exists, no 3-D
gradient or tangent array:

* NumPy in  -> low-dimensional arrays are uploaded, expanded, evaluated, shrunk, downloaded;
* torch ROCm tensors in -> zero copies.

The history dict must be of the same kind as the other arrays (NumPy history is staged per
call like the reference's in-place arrays).

``PlaneStressFrom3D`` / ``UniaxialStressFrom3D`` (no counterpart in the reference) solve, per point, for the
out-of-plane strain increments that make the constrained stresses vanish: a local Newton iteration around the
3-D law ("The f3 stress wrappers"), fused into one kernel for the same laws, and an array-level Newton
iteration around the 3-D model's own ``evaluate`` otherwise.

Around a ``UserLaw`` with an explicit or autodiff tangent all four wrappers are one launch of a kernel compiled at run time
from the law's own point function (``csrc/jit/user_law_wrapped.hip``): the strain wrappers compute the bits of
map -> evaluate -> map, the stress wrappers run the local Newton iteration per point in registers from a zero increment.
Implicit user laws take the generic path.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from .device import _check_torch, _current_stream_ptr, _is_torch
from .interfaces import IncrSmallStrainModel, StressStrainConstraint

__all__ = ["UniaxialStrainFrom3D", "PlaneStrainFrom3D", "UniaxialStressFrom3D", "PlaneStressFrom3D"]


def _has_wrapped_kernel(model) -> bool:
    """the law is a UserLaw the wrappers run as one kernel: explicit or autodiff tangent (implicit laws keep the generic path)"""
    from .userlaw import UserLaw

    return isinstance(model, UserLaw) and model.tangent_mode in ("explicit", "autodiff") and model._rotate is None


class _From3D(IncrSmallStrainModel):
    _constraint: StressStrainConstraint
    _kinds: tuple[int, int, int, int]  # grad->3d, stress->3d, stress<-3d, tangent<-3d
    #: use the fused kernel where one exists (LinearElasticityModel, the plasticity laws, user laws with an explicit or autodiff
    #: tangent); False forces map -> evaluate -> map
    fused = True

    def __init__(self, model: IncrSmallStrainModel) -> None:
        from .objective import JaumannRate

        if isinstance(model, JaumannRate):
            JaumannRate._refuse(f"{type(self).__name__} (the 2-D / 1-D wrappers)")
        assert model.constraint.name == "FULL"
        if getattr(model, "field_points", None) is not None:
            raise NotImplementedError(f"{type(self).__name__}: laws with per-point parameter fields are not supported")
        self.model = model
        self.stress_3d = None
        self.tangent_3d = None
        self.grad_del_u_3d = None

    @property
    def constraint(self) -> StressStrainConstraint:
        return self._constraint

    @property
    def history_dim(self):
        return self.model.history_dim

    def update(self) -> None:
        self.model.update()

    def _convert(self, ctx, kind, n, src, dst):
        _capi.check(ctx._lib.fcamd_convert_device(ctx.handle, kind, n, C.c_void_p(src.data_ptr()),
                                                  C.c_void_p(dst.data_ptr())))

    def evaluate(self, t, del_t, grad_del_u, stress, tangent, history) -> None:
        import torch

        gd2, sd = self.geometric_dim**2, self.stress_strain_dim
        host = not _is_torch(grad_del_u)
        if host:
            if not torch.cuda.is_available():
                raise RuntimeError("the 3D wrappers evaluate on the GPU and no HIP device is available")
            dev = torch.device("cuda", _capi.default_device())
            from .hostio import to_device

            g_lo = to_device(grad_del_u, dev, np.float64)
            s_lo = to_device(stress, dev, np.float64)
            t_lo = torch.empty(tangent.size, dtype=torch.float64, device=dev)
            h_dev = None if history is None else {k: to_device(v, dev, np.float64) for k, v in history.items()}
        else:
            g_lo, s_lo, t_lo, h_dev = (_check_torch("grad_del_u", grad_del_u), _check_torch("stress", stress),
                                       _check_torch("tangent", tangent), history)
            dev = g_lo.device
        n = g_lo.numel() // gd2
        assert n == s_lo.numel() // sd == t_lo.numel() // (sd * sd)
        if self.fused and getattr(self.model, "_model_id", None) in (_capi.LINEAR_ELASTICITY, _capi.VON_MISES_3D, _capi.COMFE_MISES_PLASTICITY,
                                                                      _capi.COMFE_DRUCKER_PRAGER, _capi.COMFE_DRUCKER_PRAGER_HYPERBOLIC):
            # fused kernel (fcamd_evaluate_device_wrapped): only the cached 3-D stress exists
            if self.stress_3d is None or self.stress_3d.numel() != 6 * n or self.stress_3d.device != dev:
                self.stress_3d = torch.zeros(6 * n, dtype=torch.float64, device=dev)
            hist = self.model._history_arrays(h_dev)
            for h in hist:
                _check_torch("history", h)
            m = self.model._handle(dev.index or 0)
            m.ctx.set_stream(_current_stream_ptr(dev.index or 0))
            m.evaluate_device_wrapped(self._constraint.value, t, del_t, n, g_lo.data_ptr(), s_lo.data_ptr(),
                                      t_lo.data_ptr(), self.stress_3d.data_ptr(), [h.data_ptr() for h in hist])
            if host:
                self.model.device_stats(dev.index or 0)  # raises on Newton non-convergence like the reference
                self._download(stress, tangent, history, s_lo, t_lo, h_dev)
            return
        if self.fused and _has_wrapped_kernel(self.model):
            # a user law with an explicit or autodiff tangent: its own fused kernel (csrc/jit/user_law_wrapped.hip), compiled on
            # first use per wrapper; only the cached 3-D stress exists.  Tensors: asynchronous, the count of failed points in
            # model.device_stats(); ndarrays: the results are downloaded, then the reference's RuntimeError is raised
            if self.stress_3d is None or self.stress_3d.numel() != 6 * n or self.stress_3d.device != dev:
                self.stress_3d = torch.zeros(6 * n, dtype=torch.float64, device=dev)
            self.model._evaluate_wrapped(self._constraint, t, del_t, g_lo, s_lo, t_lo, self.stress_3d, h_dev)
            if host:
                self._download(stress, tangent, history, s_lo, t_lo, h_dev)
                self.model._raise(self.model.device_stats(dev.index or 0))
            return
        if self.grad_del_u_3d is None or self.grad_del_u_3d.numel() != 9 * n or self.grad_del_u_3d.device != dev:
            # cached 3-D arrays (utils.py:253-266): zero-initialised once, unmapped components persist
            self.grad_del_u_3d = torch.zeros(9 * n, dtype=torch.float64, device=dev)
            self.stress_3d = torch.zeros(6 * n, dtype=torch.float64, device=dev)
            self.tangent_3d = torch.zeros(36 * n, dtype=torch.float64, device=dev)
        ctx = _capi.get_context(dev.index or 0)
        ctx.set_stream(_current_stream_ptr(dev.index or 0))
        k_g, k_s, k_sb, k_tb = self._kinds
        self._convert(ctx, k_g, n, g_lo, self.grad_del_u_3d)
        self._convert(ctx, k_s, n, s_lo, self.stress_3d)
        self._evaluate_3d(ctx, t, del_t, n, s_lo, t_lo, h_dev)
        if host:
            self._download(stress, tangent, history, s_lo, t_lo, h_dev)

    def _evaluate_3d(self, ctx, t, del_t, n, s_lo, t_lo, h_dev):
        """generic path, after the mapped components are in the cached 3-D arrays: evaluate, map back"""
        k_g, k_s, k_sb, k_tb = self._kinds
        self.model.evaluate(t, del_t, self.grad_del_u_3d, self.stress_3d, self.tangent_3d, h_dev)
        self._convert(ctx, k_tb, n, self.tangent_3d, t_lo)
        self._convert(ctx, k_sb, n, self.stress_3d, s_lo)

    @staticmethod
    def _download(stress, tangent, history, s_lo, t_lo, h_dev):
        from .hostio import assign

        assign(stress, s_lo)
        assign(tangent, t_lo)
        if history is not None:
            for k in history:
                assign(history[k], h_dev[k])


class UniaxialStrainFrom3D(_From3D):
    """Drive a 3-D model under uniaxial strain (reference ``UniaxialStrainFrom3D``,
    utils.py:211-294): component 11 of gradient, stress and tangent."""

    _constraint = StressStrainConstraint.UNIAXIAL_STRAIN
    _kinds = (_capi.GRAD_1D_TO_3D, _capi.STRESS_1D_TO_3D, _capi.STRESS_3D_TO_1D, _capi.TANGENT_3D_TO_1D)


class PlaneStrainFrom3D(_From3D):
    """Drive a 3-D model under plane strain (reference ``PlaneStrainFrom3D``, utils.py:297-412):
    gradient components (0,1,2,3)->(0,1,3,4), Mandel components 0..3, tangent block 4x4."""

    _constraint = StressStrainConstraint.PLANE_STRAIN
    _kinds = (_capi.GRAD_2D_TO_3D, _capi.STRESS_2D_TO_3D, _capi.STRESS_3D_TO_2D, _capi.TANGENT_3D_TO_2D)


# local Newton iteration of the stress wrappers: the rule of the fused kernel (kernels/stress_wrapped.h)
STRESS_WRAP_RTOL = 1e-12
STRESS_WRAP_MAX_ITER = 50


def _isotropic_tangent(kappa: float, mu: float) -> np.ndarray:
    xioi = np.zeros((6, 6))
    xioi[:3, :3] = 1.0
    return kappa * xioi + 2.0 * mu * (np.eye(6) - xioi / 3.0)


def _elastic_tangent_3d(model):
    """the 3-D law's elastic tangent (Mandel), or None where it has none independent of the state (the SLS laws: the
    local iteration then starts from a zero increment; their update is linear in it, one Newton step solves it)"""
    mid = getattr(model, "_model_id", None)
    if mid == _capi.LINEAR_ELASTICITY:
        return np.asarray(model.D, dtype=np.float64)
    if mid == _capi.VON_MISES_3D:
        return _isotropic_tangent(model.p_ka, model.p_mu)
    if mid in (_capi.COMFE_LINEAR_ELASTICITY, _capi.COMFE_MISES_PLASTICITY, _capi.COMFE_DRUCKER_PRAGER,
               _capi.COMFE_DRUCKER_PRAGER_HYPERBOLIC):
        mu, kappa = model._parameter_vector[:2]
        return _isotropic_tangent(kappa, mu)
    return None


def _solve_bb(c, r):
    """C_bb^-1 r per point, closed form (1x1 or 2x2, the kernel's expressions): c (n, k, k), r (n, k)"""
    if c.shape[1] == 1:
        return r / c[:, 0]
    c11, c12, c21, c22 = c[:, 0, 0], c[:, 0, 1], c[:, 1, 0], c[:, 1, 1]
    det = c11 * c22 - c12 * c21
    r1, r2 = r[:, 0], r[:, 1]
    import torch

    return torch.stack(((c22 * r1 - c12 * r2) / det, (c11 * r2 - c21 * r1) / det), dim=1)


class _StressFrom3D(_From3D):
    #: Mandel components whose stress is held at zero (the unknown strain increments) and their 3-D gradient entries
    _free: tuple[int, ...]
    _free_grad: tuple[int, ...]

    def _evaluate_3d(self, ctx, t, del_t, n, s_lo, t_lo, h_dev):
        """Generic path: the fused kernel's local Newton iteration as an array-level one around the 3-D model's own
        evaluate.  Every iteration starts from the committed stress and history; a point's increment is frozen once it
        has converged (or failed), so the last evaluation -- which every point takes part in -- holds every point's
        converging iterate."""
        import torch

        dev = self.stress_3d.device
        g3, s3 = self.grad_del_u_3d.view(n, 9), self.stress_3d.view(n, 6)
        tan3 = self.tangent_3d.view(n, 6, 6)
        b, gb = list(self._free), list(self._free_grad)
        s0 = s3.clone()
        h0 = None if h_dev is None else {k: v.clone() for k, v in h_dev.items()}
        ce = _elastic_tangent_3d(self.model)
        if ce is None:
            delta = torch.zeros((n, len(b)), dtype=torch.float64, device=dev)
        else:
            # C^e_bb d = -(sigma0_b + C^e_ba d_eps_a); the mapped normal strains are g[0] (and g[4] under plane stress),
            # the isotropic elastic tangents couple no shear into the normal stresses
            ce_t = torch.from_numpy(ce).to(dev)
            rhs = s0[:, b] + g3[:, 0:1] * ce_t[b, 0]
            if 1 not in b:
                rhs = rhs + g3[:, 4:5] * ce_t[b, 1]
            delta = -_solve_bb(ce_t[b][:, b].expand(n, len(b), len(b)), rhs)
        done = torch.zeros(n, dtype=torch.bool, device=dev)
        failed = torch.zeros(n, dtype=torch.bool, device=dev)
        for evals in range(1, STRESS_WRAP_MAX_ITER + 1):
            g3[:, gb] = delta
            s3.copy_(s0)
            if h0 is not None:
                for k in h_dev:
                    h_dev[k].copy_(h0[k])
            self.model.evaluate(t, del_t, self.grad_del_u_3d, self.stress_3d, self.tangent_3d, h_dev)
            r = s3[:, b]
            conv = (r == 0).all(dim=1) | (r.abs().amax(dim=1) <= STRESS_WRAP_RTOL * torch.linalg.vector_norm(s3, dim=1))
            done |= conv
            if bool(done.all()):
                break
            if evals == STRESS_WRAP_MAX_ITER:
                failed |= ~done
                break
            nd = delta - _solve_bb(tan3[:, b][:, :, b], r)
            bad = ~done & ~torch.isfinite(nd).all(dim=1)
            failed |= bad
            done |= bad
            delta = torch.where(done[:, None], delta, nd)
        if bool(failed.any()):
            raise RuntimeError(f"{type(self).__name__}: the local Newton iteration did not converge at {int(failed.sum())} points")
        self._condense(n, s_lo, t_lo)

    def _condense(self, n, s_lo, t_lo):
        s3, tan3 = self.stress_3d.view(n, 6), self.tangent_3d.view(n, 6, 6)
        if self._constraint == StressStrainConstraint.PLANE_STRESS:
            c = tan3[:, :4, :4]
            u = c[:, :, 2] / c[:, 2, 2][:, None]
            ct = c - u[:, :, None] * c[:, 2, None, :]
            ct[:, 2, :] = 0.0
            ct[:, :, 2] = 0.0
            t_lo.view(n, 4, 4).copy_(ct)
            s_lo.view(n, 4).copy_(s3[:, :4])
            s_lo.view(n, 4)[:, 2] = 0.0
        else:
            c = tan3
            c11, c12, c21, c22, c10, c20 = c[:, 1, 1], c[:, 1, 2], c[:, 2, 1], c[:, 2, 2], c[:, 1, 0], c[:, 2, 0]
            det = c11 * c22 - c12 * c21
            y1, y2 = (c22 * c10 - c12 * c20) / det, (c11 * c20 - c21 * c10) / det
            t_lo.copy_(c[:, 0, 0] - (c[:, 0, 1] * y1 + c[:, 0, 2] * y2))
            s_lo.copy_(s3[:, 0])


class UniaxialStressFrom3D(_StressFrom3D):
    """Drive a 3-D model under uniaxial stress: component 11 of gradient, stress and tangent; the lateral strain
    increments d_eps_yy, d_eps_zz are solved per point so that sigma_yy = sigma_zz = 0.  The tangent is the condensed
    d sigma_xx / d eps_xx.  Shear stresses are not enforced (they stay zero for the isotropic laws from a zero cache)."""

    _constraint = StressStrainConstraint.UNIAXIAL_STRESS
    _kinds = (_capi.GRAD_1D_TO_3D, _capi.STRESS_1D_TO_3D, _capi.STRESS_3D_TO_1D, _capi.TANGENT_3D_TO_1D)
    _free, _free_grad = (1, 2), (4, 8)


class PlaneStressFrom3D(_StressFrom3D):
    """Drive a 3-D model under plane stress: gradient components (0,1,2,3)->(0,1,3,4), Mandel components 0..3 as under
    plane strain; the out-of-plane strain increment d_eps_zz is solved per point so that sigma_zz = 0.  The returned
    sigma_zz is exactly 0 and the 4x4 tangent is the condensed one, C_aa - C_az C_zz^-1 C_za, with its zz row and column
    exactly 0.  The out-of-plane shear stresses are not enforced."""

    _constraint = StressStrainConstraint.PLANE_STRESS
    _kinds = (_capi.GRAD_2D_TO_3D, _capi.STRESS_2D_TO_3D, _capi.STRESS_3D_TO_2D, _capi.TANGENT_3D_TO_2D)
    _free, _free_grad = (2,), (8,)

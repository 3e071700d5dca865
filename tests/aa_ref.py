"""Reference for the anti-aliasing coefficient (test helper, not collected; imports no product code).

With anti-aliasing on (config.set_antialiasing, lr_set_antialiasing) preprocess stores, for every Gaussian it projects,

    record.opacity = opacity * coef,   coef = sqrt(max(0.000025, rho)),   rho = det0 / det,
    det0 = a0 c0 - b b,   det = (a0 + h)(c0 + h) - b b,   h = 0.3,

{a0, b, c0} the EWA 2D covariance BEFORE the dilation.  Everything else of the renderer reads the record, so an anti-aliased
render is, by construction, the plain renderer run on opacities `opacity * coef`.

coef32: numpy float32, operation for operation what csrc/preprocess.hip computes with FMA contraction off (every product and
        sum rounded on its own, sums left to right, GLM's column-major operator order) -- the bits the kernels produce.
coef64: torch float64, differentiable with respect to means3D and scales / rotations or cov3D, with the backward's
        convention for the 1.3 tan_fov clamp (outside it the clamped camera-space x / y is a constant; oracle/torch_oracle's
        docstring, point ii).
"""
import numpy as np
import torch

H_DILATION = 0.3
RHO_FLOOR = 0.000025


# ---------------------------------------------------------------------------------------------------------------------------
# float32, the kernel's operation order
# ---------------------------------------------------------------------------------------------------------------------------
def _f(x):
    return np.float32(x)


def _m3_mul(A, B):
    """glm::mat3 product with c[col][row] storage: R[j][i] = A[0][i] B[j][0] + A[1][i] B[j][1] + A[2][i] B[j][2]."""
    return [[(A[0][i] * B[j][0] + A[1][i] * B[j][1]) + A[2][i] * B[j][2] for i in range(3)] for j in range(3)]


def _m3_t(A):
    return [[A[i][j] for i in range(3)] for j in range(3)]


def cov2d32(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales=None, rotations=None, scale_modifier=1.0, cov3D_precomp=None):
    """(a0, b, c0, vz) float32 arrays [P]: the undilated 2D covariance as preprocess.hip forms it (forward.cu:74-152)."""
    m = np.ascontiguousarray(np.asarray(means3D, dtype=np.float32))
    V = np.asarray(viewmatrix, dtype=np.float32).reshape(16)              # flat index 4 * col + row
    P = m.shape[0]
    x, y, z = m[:, 0], m[:, 1], m[:, 2]
    zero = np.zeros(P, np.float32)
    with np.errstate(all="ignore"):
        vx = ((V[0] * x + V[4] * y) + V[8] * z) + V[12]
        vy = ((V[1] * x + V[5] * y) + V[9] * z) + V[13]
        vz = ((V[2] * x + V[6] * y) + V[10] * z) + V[14]
        if cov3D_precomp is not None:
            c3 = np.asarray(cov3D_precomp, dtype=np.float32)
            c3 = [c3[:, k] for k in range(6)]
        else:
            s = np.asarray(scales, dtype=np.float32)
            q = np.asarray(rotations, dtype=np.float32)
            mod = _f(scale_modifier)
            r, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            one, two = _f(1.0), _f(2.0)
            S = [[mod * s[:, 0], zero, zero], [zero, mod * s[:, 1], zero], [zero, zero, mod * s[:, 2]]]
            R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - r * qz), two * (qx * qz + r * qy)],
                 [two * (qx * qy + r * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - r * qx)],
                 [two * (qx * qz - r * qy), two * (qy * qz + r * qx), one - two * (qx * qx + qy * qy)]]
            Mm = _m3_mul(S, R)
            Sig = _m3_mul(_m3_t(Mm), Mm)
            c3 = [Sig[0][0], Sig[0][1], Sig[0][2], Sig[1][1], Sig[1][2], Sig[2][2]]
        tfx, tfy = _f(tanfovx), _f(tanfovy)
        focal_y = _f(H) / (_f(2.0) * tfy)                                   # rasterizer_impl.cu:223-224, in float
        focal_x = _f(W) / (_f(2.0) * tfx)
        limx, limy = _f(1.3) * tfx, _f(1.3) * tfy
        txtz, tytz = vx / vz, vy / vz
        tx = np.minimum(limx, np.maximum(-limx, txtz)) * vz
        ty = np.minimum(limy, np.maximum(-limy, tytz)) * vz
        J = [[focal_x / vz, zero, -(focal_x * tx) / (vz * vz)],
             [zero, focal_y / vz, -(focal_y * ty) / (vz * vz)],
             [zero, zero, zero]]
        b = lambda k: np.full(P, V[k], np.float32)
        Wm = [[b(0), b(4), b(8)], [b(1), b(5), b(9)], [b(2), b(6), b(10)]]
        T = _m3_mul(Wm, J)
        Vrk = [[c3[0], c3[1], c3[2]], [c3[1], c3[3], c3[4]], [c3[2], c3[4], c3[5]]]
        cov = _m3_mul(_m3_mul(_m3_t(T), _m3_t(Vrk)), T)
    return cov[0][0].astype(np.float32), cov[0][1].astype(np.float32), cov[1][1].astype(np.float32), vz.astype(np.float32)


def coef_from_cov32(a0, b, c0):
    """det0, det, rho, coef in the order of csrc/gauss_project.h aa_coef (det as preprocess forms it from the dilated entries)."""
    h = _f(H_DILATION)
    with np.errstate(all="ignore"):
        a, c = a0 + h, c0 + h
        det = a * c - b * b
        det0 = a0 * c0 - b * b
        rho = det0 / det
        coef = np.sqrt(np.fmax(_f(RHO_FLOOR), rho))          # fmaxf: a NaN rho gives the floor
    return dict(det0=det0, det=det, rho=rho, coef=coef.astype(np.float32), a=a, c=c)


def coef32(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales=None, rotations=None, scale_modifier=1.0, cov3D_precomp=None,
           full=False):
    """coef [P] float32 (1 for Gaussians behind the near plane, which preprocess never projects); full=True: the dict of
    coef_from_cov32 plus a0, b, c0, vz and `projected`."""
    n = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
    a0, b, c0, vz = cov2d32(n(means3D), n(viewmatrix), tanfovx, tanfovy, W, H, n(scales), n(rotations), scale_modifier,
                            n(cov3D_precomp))
    out = coef_from_cov32(a0, b, c0)
    projected = ~(vz <= _f(0.2))
    out["coef"] = np.where(projected, out["coef"], _f(1.0)).astype(np.float32)
    if not full:
        return out["coef"]
    out.update(a0=a0, b=b, c0=c0, vz=vz, projected=projected)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# float64, differentiable
# ---------------------------------------------------------------------------------------------------------------------------
def cov3d64(scales, rotations, scale_modifier=1.0):
    """[P, 6] upper triangle of Sigma = M^T M, M = S R (forward.cu:118-152), quaternion (r, x, y, z) used as given."""
    s = scales * scale_modifier
    r, x, y, z = rotations.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    M = R * s[:, None, :]                     # R diag(s): Sigma = R S S R^T
    Sig = M @ M.transpose(1, 2)
    return torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], dim=1)


def cov2d64(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales=None, rotations=None, scale_modifier=1.0, cov3D_precomp=None):
    """(a0, b, c0, vz) float64 tensors [P], differentiable."""
    dt = torch.float64
    m, V = means3D.to(dt), viewmatrix.to(dt).reshape(4, 4)
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    cov3D = cov3D_precomp.to(dt) if cov3D_precomp is not None else cov3d64(scales.to(dt), rotations.to(dt), scale_modifier)
    pv = m @ V[:3, :3] + V[3, :3]
    tz = pv[:, 2]
    tz_safe = torch.where(tz > 0.2, tz, torch.ones_like(tz))
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    txtz, tytz = pv[:, 0] / tz_safe, pv[:, 1] / tz_safe
    tx = torch.where((txtz < -limx) | (txtz > limx), (txtz.clamp(-limx, limx) * tz_safe).detach(), pv[:, 0])
    ty = torch.where((tytz < -limy) | (tytz > limy), (tytz.clamp(-limy, limy) * tz_safe).detach(), pv[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz_safe, zero, -(fx * tx) / (tz_safe * tz_safe),
                     zero, fy / tz_safe, -(fy * ty) / (tz_safe * tz_safe)], dim=1).reshape(-1, 2, 3)
    A = J @ V[:3, :3].T
    Sig = torch.stack([cov3D[:, 0], cov3D[:, 1], cov3D[:, 2], cov3D[:, 1], cov3D[:, 3], cov3D[:, 4],
                       cov3D[:, 2], cov3D[:, 4], cov3D[:, 5]], dim=1).reshape(-1, 3, 3)
    c2 = A @ Sig @ A.transpose(1, 2)
    return c2[:, 0, 0], c2[:, 0, 1], c2[:, 1, 1], tz


def coef_from_cov64(a0, b, c0):
    """(coef, rho, det0, det); below the floor the coefficient is the constant sqrt(floor) (zero derivative)."""
    a, c = a0 + H_DILATION, c0 + H_DILATION
    det0 = a0 * c0 - b * b
    det = a * c - b * b
    rho = det0 / det
    coef = torch.where(rho > RHO_FLOOR, torch.sqrt(rho.clamp_min(RHO_FLOOR)), torch.full_like(rho, RHO_FLOOR ** 0.5))
    return coef, rho, det0, det


def coef64(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales=None, rotations=None, scale_modifier=1.0, cov3D_precomp=None,
           full=False):
    """coef [P] float64, differentiable with respect to means3D and scales / rotations (or cov3D_precomp)."""
    a0, b, c0, vz = cov2d64(means3D, viewmatrix, tanfovx, tanfovy, W, H, scales, rotations, scale_modifier, cov3D_precomp)
    coef, rho, det0, det = coef_from_cov64(a0, b, c0)
    coef = torch.where(vz > 0.2, coef, torch.ones_like(coef))
    if full:
        return dict(coef=coef, rho=rho, det0=det0, det=det, a0=a0, b=b, c0=c0, vz=vz)
    return coef


def closed_form_cov_grads(g_rec, rec_opacity, a0, b, c0):
    """The backward of the issue / csrc/gauss_bwd.hip, float64: from g = dL/d(record opacity) and the record's opacity,
    (dL/da0, dL/db, dL/dc0) with b the single off-diagonal scalar."""
    a, c = a0 + H_DILATION, c0 + H_DILATION
    det0 = a0 * c0 - b * b
    det = a * c - b * b
    rho = det0 / det
    drho = torch.where(rho > RHO_FLOOR, g_rec * rec_opacity / (2.0 * rho), torch.zeros_like(rho))
    da0 = drho * (c0 * det - det0 * c) / (det * det)
    dc0 = drho * (a0 * det - det0 * a) / (det * det)
    db = drho * (-2.0 * b * (det - det0)) / (det * det)
    return da0, db, dc0

"""Plain torch restatement of what include/gkg_hip.h promises for the bandwidth kernels between the dense 1x1 projections
(csrc/gkg_dense.hip): train-mode BN statistics, the apply pass, the BN backward, the SyncBN split and the layout passes.

Every function computes in the dtype of its inputs.  Called with ``.double()`` operands it is the REFERENCE the GPU tests hold the
kernels to; called with the fp32 operands themselves it is the YARDSTICK ("the same formula written in plain torch fp32 ops"): the
error an honest fp32 implementation makes against the fp64 reference.  tests/test_dense_reference_host.py pins these formulas to
torch autograd of F.batch_norm(training=True) + F.gelu in double on the CPU.

Shapes: y, dy (nb, R, C); per-channel parameters (nb, C); `nb` stacks independent matrices (the groups of a grouped projection).
A helper module, not a test module and not a conftest."""
import math

import torch


# --------------------------------------------------------------------------------------------------------------- activation
def gelu(z):
    """GELU, erf form (act == 1)."""
    return z * 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))


def gelu_grad(z):
    cdf = 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))
    return cdf + z * torch.exp(-0.5 * z * z) * (1.0 / math.sqrt(2.0 * math.pi))


def act_fn(z, act):
    return gelu(z) if act == 1 else z


def act_grad(z, act):
    return gelu_grad(z) if act == 1 else torch.ones_like(z)


# --------------------------------------------------------------------------------------------------------------- forward statistics
def bn_stats(y, gamma, beta, eps):
    """Train-mode batch statistics of y (nb, R, C): biased variance, a = gamma * invstd, c = beta - a * mean (out = a*y + c).
    The variance is the two-pass (centred) one: what the shifted single-device kernel approximates."""
    mean = y.mean(1)
    var = ((y - mean[:, None, :]) ** 2).mean(1)
    return from_moments(mean, var, gamma, beta, eps)


def from_moments(mean, var, gamma, beta, eps):
    invstd = 1.0 / torch.sqrt(var + eps)
    a = gamma * invstd
    return dict(mean=mean, var=var, invstd=invstd, a=a, c=beta - a * mean)


def col_sums(y):
    """The SyncBN forward half (gkg_bn_stats_sums): plain column sum and sum of squares, [nb][2][C]."""
    return torch.stack([y.sum(1), (y * y).sum(1)], 1)


def bn_from_sums(sums, count, gamma, beta, eps):
    """gkg_bn_finalize / gkg_bn_apply_train: the statistics from (all-reduced) plain sums [nb][2][C] and the total row count."""
    mean = sums[:, 0] / count
    var = (sums[:, 1] / count - mean * mean).clamp_min(0.0)
    return from_moments(mean, var, gamma, beta, eps)


def running_update(running_mean, running_var, mean, var, bias, count, momentum):
    """The conv bias is folded into running_mean ONLY (it cancels in the output); running_var takes the unbiased estimate
    var * R / (R - 1), guarded at R == 1 (the biased one)."""
    m = mean + bias if bias is not None else mean
    unb = var * (count / (count - 1.0)) if count > 1 else var
    return (1.0 - momentum) * running_mean + momentum * m, (1.0 - momentum) * running_var + momentum * unb


# --------------------------------------------------------------------------------------------------------------- apply
def xm_cols(C, ochunk, device=None):
    """Column ch of the result lands at ch + (ch // ochunk) * ochunk: the x half of an XM buffer (ochunk == 0: identity)."""
    ch = torch.arange(C, device=device)
    return ch + (ch // ochunk) * ochunk if ochunk > 0 else ch


def row_factor(row_scale, rows_per_scale, R):
    """row_scale[r // rows_per_scale] for r in [0, R) as an (R, 1) column."""
    r = torch.arange(R, device=row_scale.device)
    return row_scale[r // rows_per_scale][:, None]


def affine_act(y, a, c, act=0, row_scale=None, rows_per_scale=1, res=None):
    """out = act(a*y + c) * row_scale[r // rows_per_scale] + res, (nb, R, C).  Also returns the magnitude of the largest
    intermediate of every element (the scale its error is measured against)."""
    ay = a[:, None, :] * y
    z = ay + c[:, None, :]
    o = act_fn(z, act)
    mag = torch.maximum(torch.maximum(ay.abs(), c[:, None, :].abs().expand_as(ay)), z.abs())
    if row_scale is not None:
        mag = torch.maximum(mag, o.abs())
        o = o * row_factor(row_scale, rows_per_scale, y.shape[1])
    if res is not None:
        mag = torch.maximum(mag, res.abs())
        o = o + res
    return o, torch.maximum(mag, o.abs())


# --------------------------------------------------------------------------------------------------------------- backward
def bn_bwd_dz(dout, y, a, c, act=0, row_scale=None, rows_per_scale=1):
    """dz = dout * row_scale[r // rows_per_scale] * act'(a*y + c)."""
    dz = dout
    if row_scale is not None:
        dz = dz * row_factor(row_scale, rows_per_scale, y.shape[1])
    if act == 1:
        dz = dz * gelu_grad(a[:, None, :] * y + c[:, None, :])
    return dz


def bn_bwd_sums(dz, y, mean, invstd):
    """[nb][2][C]: dbeta = sum dz, dgamma = sum dz * yhat, yhat = (y - mean) * invstd; and the sums of |term| (their scale)."""
    yhat = (y - mean[:, None, :]) * invstd[:, None, :]
    t = dz * yhat
    # the kernels form yhat from fp32 y and an fp32 mean: its intermediates are as large as |y| * invstd
    ymag = torch.maximum(y.abs(), mean[:, None, :].abs().expand_as(y)) * invstd[:, None, :]
    return torch.stack([dz.sum(1), t.sum(1)], 1), torch.stack([dz.abs().sum(1), (dz.abs() * ymag).sum(1)], 1)


def bn_bwd_apply(dz, y, a, mean, invstd, sums, count):
    """dy = a * (dz - sum dz / count - yhat * sum dz*yhat / count)  (count = R on one device, the total rows under SyncBN)."""
    yhat = (y - mean[:, None, :]) * invstd[:, None, :]
    return a[:, None, :] * (dz - sums[:, 0][:, None, :] / count - yhat * (sums[:, 1][:, None, :] / count))


def bn_bwd_apply_scale(dz, y, a, mean, invstd, abs_sums, count):
    """Largest intermediate of every dy element: |a| * max(|dz|, sum|dz| / count, |y| invstd * sum|dz * yhat| / count) — the two
    means carry the rounding of sums whose scale is the sum of |term|."""
    ymag = torch.maximum(y.abs(), mean[:, None, :].abs().expand_as(y)) * invstd[:, None, :]
    m = torch.maximum(dz.abs(), (abs_sums[:, 0][:, None, :] / count).expand_as(dz))
    m = torch.maximum(m, ymag * (abs_sums[:, 1][:, None, :] / count))
    return a[:, None, :].abs() * m


def bn_bwd(dout, y, a, c, mean, invstd, act=0, row_scale=None, rows_per_scale=1):
    """The whole single-device backward: dict(dz, sums [nb][2][C] = (dbeta, dgamma), abs_sums, dy, dy_scale)."""
    R = y.shape[1]
    dz = bn_bwd_dz(dout, y, a, c, act, row_scale, rows_per_scale)
    sums, abs_sums = bn_bwd_sums(dz, y, mean, invstd)
    return dict(dz=dz, sums=sums, abs_sums=abs_sums, dy=bn_bwd_apply(dz, y, a, mean, invstd, sums, R),
                dy_scale=bn_bwd_apply_scale(dz, y, a, mean, invstd, abs_sums, R))


def bn_eval_bwd(dout, y, a, c, act=0, row_scale=None, rows_per_scale=1):
    """Eval-mode BN: no batch statistic between dout and dy, dy = a * dz."""
    return a[:, None, :] * bn_bwd_dz(dout, y, a, c, act, row_scale, rows_per_scale)


def bn_eval_bwd_params(dz, y, a, running_mean, running_var, bias, eps):
    """Parameter gradients of the eval-mode BN: S0 = sum dz, S1 = sum dz * y per column;
    dbeta = S0, dgamma = (S1 + (bias - running_mean) * S0) / sqrt(running_var + eps), dbias = a * S0.
    -> dict(dgamma, dbeta, dbias) and the sums of |term| behind each (their scale)."""
    S0, S1 = dz.sum(1), (dz * y).sum(1)
    A0, A1 = dz.abs().sum(1), (dz * y).abs().sum(1)
    sh = (bias - running_mean) if bias is not None else -running_mean
    inv = 1.0 / torch.sqrt(running_var + eps)
    return (dict(dbeta=S0, dgamma=(S1 + sh * S0) * inv, dbias=a * S0),
            dict(dbeta=A0, dgamma=(A1 + sh.abs() * A0) * inv, dbias=a.abs() * A0))


# --------------------------------------------------------------------------------------------------------------- layout
def nchw_to_tm(x, img_scale=None, add_tm=None):
    """(B, C, N) -> (B*N, C) (+ add_tm), image b multiplied by img_scale[b]."""
    B, C, N = x.shape
    o = x.permute(0, 2, 1).reshape(B * N, C)
    if add_tm is not None:
        o = o + add_tm
    if img_scale is not None:
        o = (o.view(B, N, C) * img_scale[:, None, None]).reshape(B * N, C)
    return o


def tm_affine_to_nchw(y, B, C, N, a=None, c=None, res=None, img_scale=None):
    """out (B, C, N) = (a[ch] * y[t][ch] + c[ch]) * img_scale[b] + res (B, C, N).  Returns (out, largest intermediate)."""
    o = y.view(B, N, C)
    mag = o.abs()
    if a is not None:
        ay = a * o
        o = ay + c
        mag = torch.maximum(torch.maximum(ay.abs(), c.abs().expand_as(ay)), o.abs())
    if img_scale is not None:
        o = o * img_scale[:, None, None]
    o = o.permute(0, 2, 1)
    mag = mag.permute(0, 2, 1)
    if res is not None:
        mag = torch.maximum(mag, res.abs())
        o = o + res
    return o.contiguous(), torch.maximum(mag, o.abs()).contiguous()


def tm_affine_to_nchw_dual(y, B, C, N, a, c, res_tm):
    """out_tm (B*N, C) = a*y + c + res_tm (the residual given token-major) and out (B, C, N) = its transpose."""
    o = y
    mag = y.abs()
    if a is not None:
        ay = a * y
        o = ay + c
        mag = torch.maximum(torch.maximum(ay.abs(), c.abs().expand_as(ay)), o.abs())
    mag = torch.maximum(mag, res_tm.abs())
    o = o + res_tm
    mag = torch.maximum(mag, o.abs())
    return o.view(B, N, C).permute(0, 2, 1).contiguous(), o, mag


def avgpool_tm(x, B, H, W, C, r):
    """Token-major (B, H, W, C) -> (B, H//r, W//r, C): floor-mode r x r mean (rows / columns past the last full window dropped)."""
    Hr, Wr = H // r, W // r
    v = x.view(B, H, W, C)[:, :Hr * r, :Wr * r].reshape(B, Hr, r, Wr, r, C)
    return v.sum((2, 4)) / float(r * r), v.abs().sum((2, 4)) / float(r * r)

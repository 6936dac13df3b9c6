"""Row-wise kernel cases shared by tests/test_rowwise_paths_gpu.py and tests/test_rowwise_cases_cpu.py: float64 references of the norm,
element-wise, loss and optimizer kernels (csrc/norm.hip, elementwise.hip, optim.hip, the layout kernels of pooler.hip, cross-entropy of
text.hip), a float32 emulation of each arithmetic kernel in plain torch, a per-element comparator, the case tables and `paths`, the table of
cells (entry point / template instance or branch) the GPU file must reach.

bf16 inputs are exact in float64, so a reference carries only float64 error.  Where every kernel of an operation rounds an intermediate
before going on the reference rounds at the same point; today that is the RMSNorm forward alone (w * bf16(x * rstd), the HF order): its
reference hands the magnitude of the intermediate to the comparator as `pre`.

The emulations restate the kernels' operation ORDER (per-lane partial sums, the 64-lane butterfly, the per-block partials and their fold),
accumulate in float32 and store in bf16, with IEEE exp / erf / division where the kernels use v_exp_f32 / v_rcp_f32 / v_log_f32.  They share
no code with the HIP sources.  They size the bounds (BOUNDS below) and the CPU test mutates them."""
import math
import zlib
from collections import namedtuple

import torch

from gemm_cases import drop_keep, drop_params
from oracle.optim_oracle import adamw_step_ref, adan_step_ref, clip_coef

BF = torch.bfloat16
F32_MIN = 2.0 ** -126           # smallest normal float32: v_rcp_f32 and the bf16 conversion may flush what lies below it


def f32c(v):
    """a Python float as the kernel receives it (a float argument)"""
    return float(torch.tensor(v, dtype=torch.float32))


def bf16_round(x):
    return x.to(BF).double()


# ------------------------------------------------------------------------------------------------------------------------- comparator
# Per element  |got - want| <= c_out 2^-9 (|want| + pre) + c_acc 2^-24 sqrt(n) A          (bf16 outputs)
#              |got - want| <=                             c_acc 2^-24 sqrt(n) A          (fp32 outputs: stats, dgamma, dbeta, colsum,
#                                                                                          sqnorm, the loss, the optimizer state)
# 2^-9: half a bf16 ulp, the store's rounding.  `pre`: the magnitude of an intermediate that the kernel rounds to bf16 before the result is
# formed (one more half ulp of it per unit of c_out, so the c_out >= 2 measured for it grants a whole ulp: fp32 and fp64 rstd can round
# xhat to different neighbours).  A: the operation's own absolute-value accumulation, from the reference - what a relative fp32 error of
# 2^-24 per operation acts on - and n the number of terms of the longest sum behind the element (errors of a sum of n terms grow like
# sqrt(n) when they are not all of one sign).
#
# c_out = c_acc = c per output kind.  c was NOT measured on the HIP kernels: it is 4x the worst ratio |err| / (bound at c = 1) of the
# float32 EMULATION against the float64 reference over every CPU-sized case of CASES (tests/test_rowwise_cases_cpu.py recomputes the
# ratios and asserts c >= 4x each).  4x rather than the 2.5x of gemm_cases.py: the GPU evaluates exp, log, 1/x and rsqrt with ~1 ulp
# hardware approximations and contracts a*b+c to an fma, the emulation uses IEEE functions and separate roundings.
#   kind         : emulation's worst ratio at c = 1 -> c
EMU_WORST = {
    "ln_y": 1.99, "ln_stats": 0.155, "ln_dx": 1.99, "ln_dgamma": 1.1, "rms_y": 0.99, "rms_rstd": 0.0412, "rms_dx": 1.99, "rope": 2,
    "swiglu_act": 1.7, "swiglu_dgu": 1.51, "map": 2, "assemble": 2, "colsum": 0.984, "qgrad": 0.708, "ce_loss": 0.241, "ce_grad": 1.97,
    "sqnorm": 0.28, "adan": 2.33, "adamw": 2.6,
}
BOUNDS = {k: 4.0 * v for k, v in EMU_WORST.items()}

Ref = namedtuple("Ref", "want A n pre f32 alts")


def R(want, A, n=1, pre=None, f32=False, alts=None):
    """alts = (lo, hi): the only two values the element may take, bit for bit (RMSNorm forward, see ref_rmsnorm_fwd); anything else is an
    infinite error whatever the bound says"""
    return Ref(want, A, n, pre, f32, alts)


WORST = {}       # kind -> worst ratio at c = 1 seen by check() in this process

Report = namedtuple("Report", "ratio unit where")


def measure(kind, got, ref, op="", case=""):
    """-> Report(ratio = worst |err| / bound, unit = worst |err| / (the bound at c = 1), where: operation, case, row, column and values of
    the worst element).  A non-finite `got` is an infinite error."""
    want = ref.want.double()
    g = got.double().to(want.device)
    assert g.shape == want.shape, (op, case, kind, tuple(g.shape), tuple(want.shape))
    if want.dim() < 2:
        want, g = want.reshape(-1, 1), g.reshape(-1, 1)
    else:
        want, g = want.reshape(-1, want.shape[-1]), g.reshape(-1, g.shape[-1])
    A = ref.A.double().to(want.device).reshape(want.shape) if torch.is_tensor(ref.A) else torch.full_like(want, float(ref.A))
    unit = 2.0 ** -24 * math.sqrt(ref.n) * A
    if not ref.f32:
        pre = 0.0 if ref.pre is None else ref.pre.double().to(want.device).reshape(want.shape)
        unit = unit + 2.0 ** -9 * (want.abs() + pre)
    err = (g - want).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    r1 = torch.where(err == 0, torch.zeros_like(err), err / unit.clamp_min(1e-300))
    if ref.alts is not None:
        lo, hi = (a.double().to(want.device).reshape(want.shape) for a in ref.alts)
        r1 = torch.where((g == lo) | (g == hi), r1, torch.full_like(r1, float("inf")))
    i = int(r1.reshape(-1).nan_to_num(float("inf")).argmax())
    row, col = divmod(i, want.shape[1])
    u = float(r1.reshape(-1)[i])
    ratio = u / BOUNDS[kind]
    where = (f"{op} [{case}] {kind}: row {row} col {col} got {float(g[row, col]):.9g} want {float(want[row, col]):.9g}, "
             f"{ratio:.3g}x its bound ({u:.3g} at c = 1, c = {BOUNDS[kind]:.3g})")
    return Report(ratio, u, where)


def check(kind, got, ref, op="", case=""):
    rep = measure(kind, got, ref, op, case)
    WORST[kind] = max(WORST.get(kind, 0.0), rep.unit)
    assert rep.ratio <= 1.0, rep.where
    return rep


# ------------------------------------------------------------------------------------------------------------------------- references
def _d(*ts):
    return [None if t is None else t.double() for t in ts]


def ref_layernorm_fwd(x, gamma, beta, eps):
    x, g, b = _d(x, gamma, beta)
    cols = x.shape[1]
    mean = x.mean(1)
    d = x - mean[:, None]
    rstd = ((d * d).mean(1) + f32c(eps)).rsqrt()
    mabs = x.abs().mean(1)
    y = d * rstd[:, None] * g + b
    A = g.abs() * rstd[:, None] * (d.abs() + mabs[:, None]) + b.abs()
    return dict(y=R(y, A, cols), mean=R(mean, mabs, cols, f32=True), rstd=R(rstd, rstd, cols, f32=True))


def ref_layernorm_bwd(dy, x, gamma, mean, rstd, add=None, old=None, need_dx=True, need_dg=True):
    """mean / rstd: the saved fp32 statistics, exact inputs here.  old = (dgamma, dbeta) before the call when accumulate."""
    dy, x, g, mu, rs, add = _d(dy, x, gamma, mean, rstd, add)
    rows, cols = x.shape
    xh = (x - mu[:, None]) * rs[:, None]
    gd = g * dy
    out = {}
    if need_dx:
        s1, s2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
        S1, S2 = gd.abs().mean(1, keepdim=True), (gd * xh).abs().mean(1, keepdim=True)
        dx = rs[:, None] * (gd - s1 - xh * s2)
        A = rs[:, None] * (gd.abs() + S1 + xh.abs() * S2)
        if add is not None:
            dx, A = dx + add, A + add.abs()
        out["dx"] = R(dx, A, cols)
    if need_dg:
        dg, Ag, db, Ab = (dy * xh).sum(0), (dy * xh).abs().sum(0), dy.sum(0), dy.abs().sum(0)
        if old is not None:
            dg, Ag, db, Ab = dg + old[0].double(), Ag + old[0].double().abs(), db + old[1].double(), Ab + old[1].double().abs()
        out["dgamma"], out["dbeta"] = R(dg, Ag, rows, f32=True), R(db, Ab, rows, f32=True)
    return out


def ref_rmsnorm_fwd(x, w, eps):
    x, w = _d(x, w)
    cols = x.shape[1]
    rstd = ((x * x).mean(1) + f32c(eps)).rsqrt()
    xh = x * rstd[:, None]
    y = w * bf16_round(xh)                                 # the HF order: xhat rounded to the activation type, then the weight
    pre = (w * xh).abs()
    # The kernel's xhat is fl32(x * rstd32): within tol of x * rstd relatively (the bound on rstd plus one fp32 rounding).  Rounding is
    # monotone, so its bf16 value lies between the roundings of the two ends of that interval - which coincide unless x * rstd is that close
    # to a tie - and w * bf16(xhat) is exact in fp32 (two 8-bit significands), stored with one rounding: the result is one of two known bf16
    # values, almost everywhere one.
    tol = BOUNDS["rms_rstd"] * 2.0 ** -24 * math.sqrt(cols) + 2.0 ** -23
    alts = tuple(bf16_round(w * bf16_round(xh * f)) for f in (1 - tol, 1 + tol))
    return dict(y=R(y, pre, cols, pre=pre, alts=alts), rstd=R(rstd, rstd, cols, f32=True))


def ref_rmsnorm_bwd(dy, x, w, rstd=None, add=None, eps=1e-5):
    dy, x, w, rs, add = _d(dy, x, w, rstd, add)
    cols = x.shape[1]
    if rs is None:
        rs = ((x * x).mean(1) + f32c(eps)).rsqrt()
    xh, gd = x * rs[:, None], w * dy
    s, S = (gd * xh).mean(1, keepdim=True), (gd * xh).abs().mean(1, keepdim=True)
    dx = rs[:, None] * (gd - xh * s)
    A = rs[:, None] * (gd.abs() + xh.abs() * S)
    if add is not None:
        dx, A = dx + add, A + add.abs()
    return dict(dx=R(dx, A, cols))


def rope_tables(npos, D, device="cpu"):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    f = torch.outer(torch.arange(npos, dtype=torch.float64), inv)
    return f.cos().float().to(device), f.sin().float().to(device)


def ref_rope(x, cos_t, sin_t, pos, nheads, D, inverse=False):
    """x [rows, nheads * D]; pos int64 [rows]; rotate_half convention"""
    x = x.double().reshape(x.shape[0], nheads, D)
    h = D // 2
    c, s = cos_t.double()[pos][:, None, :], sin_t.double()[pos][:, None, :] * (-1.0 if inverse else 1.0)
    a, b = x[..., :h], x[..., h:]
    want = torch.cat([a * c - b * s, b * c + a * s], -1)
    A = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
    return dict(x=R(want.reshape(x.shape[0], -1), A.reshape(x.shape[0], -1)))


def ref_swiglu_fwd(gu, F):
    g, u = gu.double()[:, :F], gu.double()[:, F:2 * F]
    want = g * torch.sigmoid(g) * u
    # exp(-g) carries a relative error ~|g| 2^-24 (the argument's scaling); a sigmoid below the smallest normal fp32 may be flushed
    A = want.abs() * (1 + g.abs()) + (g * u).abs() * (F32_MIN * 2.0 ** 24)
    return dict(act=R(want, A))


def ref_swiglu_bwd(dact, gu, F):
    d, g, u = dact.double(), gu.double()[:, :F], gu.double()[:, F:2 * F]
    sg = torch.sigmoid(g)
    du, dg = d * g * sg, d * u * sg * (1 + g * (1 - sg))
    flush = F32_MIN * 2.0 ** 24
    Au = du.abs() * (1 + g.abs()) + (d * g).abs() * flush
    Ag = (d * u).abs() * sg * (1 + g.abs() * (1 - sg)) * (1 + g.abs()) + (d * u).abs() * (1 + g.abs()) * flush
    return dict(dgu=R(torch.cat([dg, du], 1), torch.cat([Ag, Au], 1)))


def ref_map(op, a, b=None):
    a, b = _d(a, b)
    if op == 0:
        erf = torch.erf(a * 0.7071067811865476)
        return dict(out=R(0.5 * a * (1 + erf), 0.5 * a.abs() * (1 + erf.abs())))
    if op == 1:        # a = dY, b = the pre-activation
        cdf = 0.5 * (1 + torch.erf(b * 0.7071067811865476))
        pdf = 0.3989422804014327 * torch.exp(-0.5 * b * b)
        return dict(out=R(a * (cdf + b * pdf), a.abs() * (1 + b.abs() * pdf * (1 + 0.5 * b * b))))
    if op == 2:
        return dict(out=R(a + b, a.abs() + b.abs()))
    if op == 3:
        want = a * torch.sigmoid(1.702 * a)
        return dict(out=R(want, want.abs() * (1 + 1.702 * a.abs()) + a.abs() * (F32_MIN * 2.0 ** 24)))
    raise ValueError(op)


def ref_assemble(patch, cls, pos, B, NP):
    patch, cls, pos = _d(patch, cls, pos)
    dim = patch.shape[1]
    tok = torch.cat([cls.reshape(1, 1, dim).expand(B, 1, dim), patch.reshape(B, NP, dim)], 1)
    return dict(out=R((tok + pos[None]).reshape(-1, dim), (tok.abs() + pos[None].abs()).reshape(-1, dim)))


def ref_colsum(x, old=None):
    x = x.double()
    s, A = x.sum(0), x.abs().sum(0)
    if old is not None:
        s, A = s + old.double(), A + old.double().abs()
    return dict(out=R(s, A, x.shape[0], f32=True))


def ref_sqnorm(g, old=None):
    g = g.double()
    s = (g * g).sum().reshape(1)
    want = s if old is None else s + old.double().reshape(1)
    return dict(out=R(want, want.abs(), g.numel(), f32=True))


def query_rows(nq, ni):
    """row of kv[b] that holds query r (kv[b] = [q_g0 | img_g0 | q_g1 | img_g1 | q_g2 | img_g2])"""
    rows, kvo = [], 0
    for q, i in zip(nq, ni):
        rows += [kvo + j for j in range(q)]
        kvo += q + i
    return rows


def ref_pooler_build(query, img, B, nq, ni):
    """-> (t [B * NQ, dim], kv [B * KV, dim]) by torch.cat (bit-exact layout restatement)"""
    NI = sum(ni)
    img = img.reshape(B, NI, -1)
    t = torch.cat([query] * B, 0)
    parts = []
    for b in range(B):
        qo = io = 0
        for q, i in zip(nq, ni):
            parts += [query[qo:qo + q], img[b, io:io + i]]
            qo, io = qo + q, io + i
    return t, torch.cat(parts, 0)


def ref_query_grad(dt0, dkv, B, nq, ni, old=None):
    NQ, KV = sum(nq), sum(nq) + sum(ni)
    d = dt0.double().reshape(B, NQ, -1)
    s, A, n = d.sum(0), d.abs().sum(0), B
    if dkv is not None:
        k = dkv.double().reshape(B, KV, -1)[:, query_rows(nq, ni)]
        s, A, n = s + k.sum(0), A + k.abs().sum(0), 2 * B
    if old is not None:
        s, A = s + old.double(), A + old.double().abs()
    return dict(out=R(s, A, n, f32=True))


def ref_ce(logits, target):
    x = logits.double()
    n, V = x.shape
    lse = torch.logsumexp(x, 1)
    xt = x.gather(1, target.long()[:, None])[:, 0]
    row = lse - xt
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x).scatter_(1, target.long()[:, None], 1.0)
    A_row = lse.abs() + xt.abs() + 1
    return dict(row_loss=R(row, A_row, V, f32=True), loss=R(row.mean().reshape(1), A_row.mean().reshape(1), V, f32=True),
                grad=R((p - onehot) / n, (p * (1 + x.abs() + lse.abs()[:, None]) + onehot + F32_MIN * 2.0 ** 24) / n, V))   # + a flushed exp


def _state64(st):
    return {k: (None if v is None else v.double().clone()) for k, v in st.items()}


def ref_adan(st, g, step, lr, betas, eps, wd, no_prox, clip, max_norm, grad_scale):
    """One Adan step from the fp32 state `st` = dict(p, m, v, n, pre) (pre None at step 1) by oracle/optim_oracle.py in float64.  clip: the
    kernel is handed the squared norm of g.  -> {name: Ref}.  A: first-order propagation of a relative 2^-24 per operation through the
    update (the cancellations g - pre and m/bc1 + b2 v/bc2, the division by sqrt(n)/sqrt(bc3) + eps)."""
    b1, b2, b3 = betas
    lr, eps, wd, gs, mn = f32c(lr), f32c(eps), f32c(wd), f32c(grad_scale), f32c(max_norm)
    s0 = _state64(st)
    g64 = g.double() * gs
    use_clip = clip and mn > 0
    new = adan_step_ref(_state64(st), g64, step, lr, tuple(f32c(b) for b in betas), eps, wd, no_prox, mn if use_clip else 0.0)
    gc = g64 * (clip_coef(g64, mn) if use_clip else 1.0)
    pg = gc if s0["pre"] is None else s0["pre"]
    bc1, bc2, bc3s = 1 - b1 ** step, 1 - b2 ** step, math.sqrt(1 - b3 ** step)
    Ad = gc.abs() + pg.abs()
    Am, Av = s0["m"].abs() + gc.abs(), s0["v"].abs() + Ad
    u = gc + b2 * (gc - pg)
    An = new["n"] + 2 * (1 - b3) * u.abs() * (gc.abs() + b2 * Ad)
    rn = new["n"].sqrt()
    denom = rn / bc3s + eps
    upd = (new["m"] / bc1 + b2 * new["v"] / bc2) / denom
    Ap = s0["p"].abs() + lr * ((Am / bc1 + b2 * Av / bc2) / denom + upd.abs() * An / (2 * rn * bc3s * denom).clamp_min(1e-300))
    n = g.numel() if use_clip else 1
    return {"p": R(new["p"], Ap, n, f32=True), "m": R(new["m"], Am, n, f32=True), "v": R(new["v"], Av, n, f32=True),
            "n": R(new["n"], An, n, f32=True), "pre": R(new["pre"], gc.abs(), n, f32=True)}


def ref_adamw(st, g, step, lr, betas, eps, wd, clip, max_norm, grad_scale):
    b1, b2 = betas
    lr, eps, wd, gs, mn = f32c(lr), f32c(eps), f32c(wd), f32c(grad_scale), f32c(max_norm)
    s0 = _state64(st)
    g64 = g.double() * gs
    use_clip = clip and mn > 0
    new = adamw_step_ref(_state64(st), g64, step, lr, tuple(f32c(b) for b in betas), eps, wd, mn if use_clip else 0.0)
    gc = g64 * (clip_coef(g64, mn) if use_clip else 1.0)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    Am = s0["m"].abs() + gc.abs()
    Av = s0["v"].abs() + 3 * (1 - b2) * gc * gc
    rv = new["v"].sqrt()
    denom = rv / math.sqrt(bc2) + eps
    Ap = s0["p"].abs() + (lr / bc1) * (Am / denom + new["m"].abs() / denom ** 2 * Av / (2 * rv * math.sqrt(bc2)).clamp_min(1e-300))
    n = g.numel() if use_clip else 1
    return {"p": R(new["p"], Ap, n, f32=True), "m": R(new["m"], Am, n, f32=True), "v": R(new["v"], Av, n, f32=True)}


# ------------------------------------------------------------------------------------------------------------------------- emulations
# float32 torch on the CPU.  `mut`: a named defect (tests/test_rowwise_cases_cpu.py); None is the kernel as written.
_XOR = {o: torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)}


def _wave_sum(v):
    """the 64-lane xor butterfly of wave_sum on the last dimension"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _XOR[o]]
    return v


def _row_sum(t):
    """[rows, cols] -> [rows]: lane l adds its 8 values of each 512-column chunk in order, then the butterfly"""
    rows, cols = t.shape
    v = t.reshape(rows, cols // 512, 64, 8)
    s = torch.zeros(rows, 64)
    for c in range(cols // 512):
        for i in range(8):
            s = s + v[:, c, :, i]
    return _wave_sum(s)[:, 0]


def _block_sum(v):
    """block_sum<4> over [..., 256] -> [...]"""
    w = _wave_sum(v.reshape(*v.shape[:-1], 4, 64))[..., 0]
    t = torch.zeros(v.shape[:-1])
    for i in range(4):
        t = t + w[..., i]
    return t


def _strided_sum(v, T):
    """[n] -> [T]: thread t adds v[t], v[t + T], ... in order"""
    K = -(-v.numel() // T)
    p = torch.zeros(K * T)
    p[:v.numel()] = v
    p = p.reshape(K, T)
    s = torch.zeros(T)
    for k in range(K):
        s = s + p[k]
    return s


def emu_layernorm_fwd(x, gamma, beta, eps, mut=None):
    x, g, b = x.float(), gamma.float(), beta.float()
    cols = x.shape[1]
    inv = torch.tensor(1.0 / (cols - 1 if mut == "mean_over_cols_minus_1" else cols), dtype=torch.float32)
    mean = _row_sum(x) * inv
    d = x - mean[:, None]
    var = _row_sum(d * d) * inv
    rstd = 1.0 / torch.sqrt(var if mut == "eps_omitted" else var + torch.tensor(eps, dtype=torch.float32))
    y = (x - mean[:, None]) * rstd[:, None] * g + b
    return dict(y=y.to(BF), mean=mean, rstd=rstd)


def layernorm_bwd_nblk(rows):
    return min(-(-rows // 4), 256)


def _ln_partials(t, nblk, drop_last_row=False):
    """[rows, cols] -> [cols]: (block, wave) adds rows blk*4 + w, + nblk*4, ... in order; the 4 waves of a block are added in order; finalize
    slice s adds blocks s, s + 8, ... in order, then the 8 slices in order"""
    rows, cols = t.shape
    if drop_last_row:
        t = t.clone()
        t[rows - 1] = 0
    stride = nblk * 4
    K = -(-rows // stride)
    p = torch.zeros(K * stride, cols)
    p[:rows] = t
    p = p.reshape(K, nblk, 4, cols)
    acc = torch.zeros(nblk, 4, cols)
    for k in range(K):
        acc = acc + p[k]
    part = acc[:, 0] + acc[:, 1] + acc[:, 2] + acc[:, 3]
    K2 = -(-nblk // 8)
    q = torch.zeros(K2 * 8, cols)
    q[:nblk] = part
    q = q.reshape(K2, 8, cols)
    a = torch.zeros(8, cols)
    for k in range(K2):
        a = a + q[k]
    s = torch.zeros(cols)
    for i in range(8):
        s = s + a[i]
    return s


def emu_layernorm_bwd(dy, x, gamma, mean, rstd, add=None, old=None, need_dx=True, need_dg=True, mut=None):
    dy, x, g = dy.float(), x.float(), gamma.float()
    rows, cols = x.shape
    inv = torch.tensor(1.0 / cols, dtype=torch.float32)
    xh = (x - mean[:, None]) * rstd[:, None]
    gd = g * dy
    out = {}
    if need_dx:
        s1, s2 = _row_sum(gd) * inv, _row_sum(gd * xh) * inv
        dx = rstd[:, None] * (g * dy - s1[:, None] - xh * s2[:, None])
        if add is not None and mut != "add_dropped":
            dx = dx + add.float()
        out["dx"] = dx.to(BF)
    if need_dg:
        nblk = layernorm_bwd_nblk(rows)
        dg = _ln_partials(dy * xh, nblk, drop_last_row=(mut == "last_row_missing_from_dgamma"))
        db = _ln_partials(dy, nblk)
        if mut == "dbeta_dgamma_swapped":
            dg, db = db, dg
        if old is not None and mut != "accumulate_ignored":
            dg, db = old[0] + dg, old[1] + db
        out["dgamma"], out["dbeta"] = dg, db
    return out


def emu_rmsnorm_fwd(x, w, eps, mut=None):
    x, w = x.float(), w.float()
    cols = x.shape[1]
    q = _row_sum(x * x) * torch.tensor(1.0 / cols, dtype=torch.float32)
    rstd = 1.0 / torch.sqrt(q if mut == "eps_omitted" else q + torch.tensor(eps, dtype=torch.float32))
    xh = x * rstd[:, None]
    if mut != "xhat_not_rounded":
        xh = xh.to(BF).float()
    return dict(y=(w * xh).to(BF), rstd=rstd)


def emu_rmsnorm_bwd(dy, x, w, rstd=None, add=None, eps=1e-5, mut=None):
    dy, x, w = dy.float(), x.float(), w.float()
    cols = x.shape[1]
    inv = torch.tensor(1.0 / cols, dtype=torch.float32)
    if rstd is None:
        rstd = 1.0 / torch.sqrt(_row_sum(x * x) * inv + torch.tensor(eps, dtype=torch.float32))
    xh, gd = x * rstd[:, None], dy * w
    s = _row_sum(gd * xh) * inv
    dx = rstd[:, None] * (gd - xh * s[:, None])
    if add is not None and mut != "add_dropped":
        dx = dx + add.float()
    return dict(dx=dx.to(BF))


def emu_rope(x, cos_t, sin_t, pos, nheads, D, inverse=False, mut=None):
    rows = x.shape[0]
    x = x.float().reshape(rows, nheads, D)
    h = D // 2
    if mut == "position_off_by_one":
        pos = pos + 1
    c, s = cos_t[pos][:, None, :], sin_t[pos][:, None, :] * (-1.0 if inverse else 1.0)
    a, b = x[..., :h], x[..., h:]
    o1 = a * c - b * s
    o2 = b * c + a * (-s if mut == "sin_sign_flipped_on_second_half" else s)
    return dict(x=torch.cat([o1, o2], -1).reshape(rows, -1).to(BF))


def _sigmoid32(x):
    return 1.0 / (1.0 + torch.exp(-x))


def emu_swiglu_fwd(gu, F, mut=None):
    g, u = gu.float()[:, :F], gu.float()[:, F:2 * F]
    return dict(act=((g * _sigmoid32(g)) * u).to(BF))


def emu_swiglu_bwd(dact, gu, F, mut=None):
    d, g, u = dact.float(), gu.float()[:, :F], gu.float()[:, F:2 * F]
    sg = _sigmoid32(g)
    du = d * g * sg
    dg = d * u * sg * (1.0 + g * (1.0 - sg))
    if mut == "du_dg_swapped":
        du, dg = dg, du
    return dict(dgu=torch.cat([dg, du], 1).to(BF))


def emu_map(op, a, b=None, mut=None):
    a = a.float()
    b = None if b is None else b.float()
    if op == 0:
        out = 0.5 * a * (1.0 + torch.erf(a * 0.70710678118654752))
    elif op == 1:
        if mut == "gelu_bwd_tanh_form":
            k = 0.7978845608028654
            t = torch.tanh(k * (b + 0.044715 * b ** 3))
            out = a * (0.5 * (1 + t) + 0.5 * b * (1 - t * t) * k * (1 + 3 * 0.044715 * b * b))
        else:
            cdf = 0.5 * (1.0 + torch.erf(b * 0.70710678118654752))
            pdf = 0.3989422804014327 * torch.exp(-0.5 * b * b)
            out = a * (cdf + b * pdf)
    elif op == 2:
        out = a + b
    else:
        out = a * _sigmoid32(1.702 * a)
    return dict(out=out.to(BF))


def emu_assemble(patch, cls, pos, B, NP, mut=None):
    dim = patch.shape[1]
    tok = torch.cat([cls.float().reshape(1, 1, dim).expand(B, 1, dim), patch.float().reshape(B, NP, dim)], 1)
    return dict(out=(tok + pos.float()[None]).reshape(-1, dim).to(BF))


def colsum_nsplit(rows):
    return max(1, min(-(-rows // 256), 64))


def emu_colsum(x, old=None, mut=None):
    x = x.float()
    rows, cols = x.shape
    ns = colsum_nsplit(rows)
    per = -(-rows // ns)
    out = torch.zeros(cols)
    for k in range(ns):
        r0, r1 = k * per, min(rows, (k + 1) * per)
        if mut == "last_row_of_one_split_dropped" and k == ns // 2:
            r1 -= 1
        n = max(r1 - r0, 0)
        K = -(-n // 4)
        p = torch.zeros(K * 4, cols)
        p[:n] = x[r0:r0 + n]
        p = p.reshape(K, 4, cols)
        acc = torch.zeros(4, cols)
        for j in range(K):
            acc = acc + p[j]
        out = out + (acc[0] + acc[1] + acc[2] + acc[3])
    return dict(out=out if old is None else old + out)


def sqnorm_nblk(n):
    return max(1, min(-(-n // 256), 4096))


def emu_sqnorm(g, old=None, mut=None):
    g = g.float().reshape(-1)
    if mut == "tail_beyond_multiple_of_256_dropped":
        g = g[:g.numel() // 256 * 256]
    nb = sqnorm_nblk(g.numel())
    part = _block_sum(_strided_sum(g * g, nb * 256).reshape(nb, 256))
    s = _block_sum(_strided_sum(part, 256))
    return dict(out=(s if old is None else old.reshape(()) + s).reshape(1))


def emu_query_grad(dt0, dkv, B, nq, ni, old=None, mut=None):
    NQ, KV = sum(nq), sum(nq) + sum(ni)
    d = dt0.float().reshape(B, NQ, -1)
    k = None if dkv is None else dkv.float().reshape(B, KV, -1)[:, query_rows(nq, ni)]
    s = torch.zeros_like(d[0])
    for b in range(B):
        s = s + d[b]
        if k is not None:
            s = s + k[b]
    return dict(out=s if old is None or mut == "accumulate_ignored" else old + s)


def emu_ce(logits, target, mut=None):
    """ce_kernel: 256 threads walk the V / 8 chunks of a row with an online (max, sum); block max, block sum; the gradient pass"""
    x = logits.float()
    n, V = x.shape
    nch = V // 8
    Rn = -(-nch // 256)
    xc = torch.full((n, Rn * 256, 8), float("nan"))
    xc[:, :nch] = x.reshape(n, nch, 8)
    xc = xc.reshape(n, Rn, 256, 8)
    ninf = float("-inf")
    m, s = torch.full((n, 256), ninf), torch.zeros(n, 256)
    for r in range(Rn):
        v = xc[:, r]
        valid = (r * 256 + torch.arange(256) < nch)[None, :]
        mn = torch.maximum(m, v.max(-1).values)
        if mut == "no_max_subtraction":
            mn = torch.zeros_like(mn)
        acc = torch.zeros(n, 256)
        for i in range(8):
            acc = acc + torch.exp(v[..., i] - mn)
        s_new = s * torch.exp(m - mn) + acc                      # a first chunk: m = -inf, s = 0 -> 0 * exp(-inf) = 0
        s, m = torch.where(valid, s_new, s), torch.where(valid, mn, m)
    M = m.max(1).values
    ssum = _block_sum(s * torch.exp(m - M[:, None]))
    lse = M + torch.log(ssum)
    t = target.long()
    row = lse - x.gather(1, t[:, None])[:, 0]
    hot = (t + 1) % V if mut == "onehot_at_t_plus_1" else t
    onehot = torch.zeros_like(x).scatter_(1, hot[:, None], 1.0)
    scale = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float((n - 1) if mut == "grad_scaled_by_1_over_n_minus_1" else n), dtype=torch.float32)
    grad = ((torch.exp(x - lse[:, None]) - onehot) * scale).to(BF)
    loss = _block_sum(_strided_sum(row, 256)) * torch.tensor(1.0 / n, dtype=torch.float32)
    return dict(row_loss=row, loss=loss.reshape(1), grad=grad)


def _emu_coef(g, clip, max_norm, grad_scale, mut=None):
    gs = torch.tensor(grad_scale, dtype=torch.float32)
    if not clip or max_norm <= 0:
        return gs
    norm = torch.sqrt(emu_sqnorm(g)["out"][0]) * gs
    c = torch.tensor(max_norm, dtype=torch.float32) / (norm + torch.tensor(1e-6, dtype=torch.float32))
    if mut != "clip_applied_when_coef_above_1":
        c = torch.clamp(c, max=1.0)
    return c * gs


def _t(v):
    return torch.tensor(v, dtype=torch.float32)


def emu_adan(st, g, step, lr, betas, eps, wd, no_prox, clip, max_norm, grad_scale, mut=None):
    b1, b2, b3 = (_t(b) for b in betas)
    lr, eps, wd, one = _t(lr), _t(eps), _t(wd), _t(1.0)
    bstep = step - 1 if mut == "bias_correction_with_step_minus_1" else step
    bc1, bc2 = one - torch.pow(b1, _t(float(bstep))), one - torch.pow(b2, _t(float(bstep)))
    bc3s = torch.sqrt(one - torch.pow(b3, _t(float(bstep))))
    gg = g * _emu_coef(g, clip, max_norm, grad_scale, mut)
    pg = gg if step == 1 else st["pre"]
    diff = gg - pg
    m = st["m"] + (gg - st["m"]) * (one - b1)
    v = st["v"] + (diff - st["v"]) * (one - b2)
    u = gg + b2 * diff
    nn = st["n"] * b3 + u * u * (one - b3)
    denom = torch.sqrt(nn) / bc3s + eps
    upd = (m / bc1 + b2 * v / bc2) / denom
    w = st["p"] * (one - lr * wd) - lr * upd if no_prox else (st["p"] - lr * upd) / (one + lr * wd)
    pre = (st["pre"] if st["pre"] is not None else torch.zeros_like(g)) if mut == "pre_grad_not_updated" else gg
    return dict(p=w, m=m, v=v, n=nn, pre=pre, shadow=w.to(BF))


def emu_adamw(st, g, step, lr, betas, eps, wd, clip, max_norm, grad_scale, mut=None):
    b1, b2 = (_t(b) for b in betas)
    lr, eps, wd, one = _t(lr), _t(eps), _t(wd), _t(1.0)
    bc1, bc2 = one - torch.pow(b1, _t(float(step))), one - torch.pow(b2, _t(float(step)))
    gg = g * _emu_coef(g, clip, max_norm, grad_scale, mut)
    w = st["p"]
    if mut == "coupled_l2":
        gg = gg + wd * w
    m = b1 * st["m"] + (one - b1) * gg
    v = b2 * st["v"] + (one - b2) * gg * gg
    denom = torch.sqrt(v) / torch.sqrt(bc2) + eps
    w = (w if mut == "coupled_l2" else w * (one - lr * wd)) - (lr / bc1) * (m / denom)
    return dict(p=w, m=m, v=v, shadow=w.to(BF))


def ref_dropout(x, p, seed):
    """bit-exact: kept elements bf16(x * scale) in fp32 arithmetic, dropped ones +0; element index row * cols + col"""
    rows, cols = x.shape
    thresh, scale = drop_params(p)
    idx = torch.arange(rows, device=x.device, dtype=torch.int64)[:, None] * cols + torch.arange(cols, device=x.device, dtype=torch.int64)[None, :]
    keep = drop_keep(seed, idx, thresh)
    y = (x.float() * torch.tensor(scale, dtype=torch.float32, device=x.device)).to(BF)
    return torch.where(keep, y, torch.zeros_like(y)), keep


# ------------------------------------------------------------------------------------------------------------------------- cells
GRID_CAP, OPT_CAP = 8192 * 256, 4096 * 256          # grid_for / ogrid: blocks x threads; beyond them a thread takes a second trip


def _grid(work):
    return "grid_stride" if work > GRID_CAP else "one_trip"


def cells_of(op, shape, opt):
    """The cells one case covers, from the host rules: cols / 512 names the norm instance, the four caps (grid_for 8192 blocks, ogrid 4096
    blocks, lhrs_layernorm_bwd_nblk 256 blocks of 4 rows, lhrs_colsum_nsplit 64 splits of 256 rows) the grid-stride trips, NULL options
    the branches."""
    s, o = shape, opt
    c = set()
    if op in ("layernorm_fwd", "rmsnorm_fwd", "rmsnorm_fwd_q", "rmsnorm_bwd", "rmsnorm_bwd_q", "layernorm_bwd"):
        c.add(f"NCH={s['cols'] // 512}")
        if s["rows"] % 4:
            c.add("partial_block")
    if op == "layernorm_fwd":
        c |= {"stats" if o.get("stats") else "no_stats"} | ({"strided"} if o.get("strided") else set())
    elif op == "layernorm_bwd":
        c.add("grid_stride" if s["rows"] > 1024 else "one_trip")
        c.add("dgamma" if o.get("dgamma", True) else "no_dgamma")
        c.add("dx" if o.get("need_dx", True) else "no_dx")
        c.add({None: "no_add", "separate": "add", "alias": "add_alias"}[o.get("add")])
        c |= {k for k in ("accumulate", "strided", "nan_workspace") if o.get(k)}
    elif op == "rmsnorm_fwd":
        c |= {"rstd" if o.get("rstd") else "no_rstd"} | ({"strided"} if o.get("strided") else set())
    elif op == "rmsnorm_fwd_q":
        c.add("y" if o.get("y", True) else "no_y")
    elif op in ("rmsnorm_bwd", "rmsnorm_bwd_q"):
        c.add("rstd" if o.get("rstd") else "recompute")
        c.add({None: "no_add", "separate": "add", "alias": "add_alias"}[o.get("add")])
        if o.get("dy_alias"):
            c.add("dy_alias")
    elif op == "rope":
        c |= {f"D={s['D']}", "pos_ids" if o.get("pos_ids") else "pos_mod", _grid(s["rows"] * s["nheads"] * (s["D"] // 16))}
        c |= {k for k in ("pos0", "inverse", "strided") if o.get(k)}
    elif op in ("swiglu_fwd", "swiglu_bwd"):
        c.add(_grid(s["rows"] * (s["F"] // 8)))
        if o.get("alias"):
            c.add("alias")
    elif op == "map":
        c |= {f"op{o['op']}", _grid(s["n"] // 8)} | ({"alias"} if o.get("alias") else set())
    elif op == "dropout":
        c |= {"p0" if o["p"] == 0 else "p"} | ({"strided"} if o.get("strided") else set())
    elif op == "colsum":
        ns = colsum_nsplit(s["rows"])
        c.add("nsplit=1" if ns == 1 else "nsplit_cap" if s["rows"] > 64 * 256 else "nsplit>1")
        c |= {k for k in ("accumulate", "strided") if o.get(k)}
    elif op == "transpose":
        c.add("pad" if s["rows_pad"] > s["rows"] else "no_pad")
    elif op in ("gather_rows", "scatter_rows"):
        c.add("multi_trip" if s["dim"] // 8 > 256 else "one_trip")
    elif op == "pooler_query_grad":
        c |= {"dkv" if o.get("dkv", True) else "no_dkv"} | ({"accumulate"} if o.get("accumulate") else set())
    elif op == "ce":
        nch = s["V"] // 8
        c.add("idle_threads" if nch < 256 else "multi_trip" if nch > 256 else "one_trip")
        c |= {"no_grad" if not o.get("grad", True) else "inplace" if o.get("inplace", True) else "out_of_place"}
        if o.get("strided"):
            c.add("strided")
    elif op == "sqnorm":
        c |= {"grid_stride" if s["n"] > OPT_CAP else "one_block" if s["n"] <= 256 else "blocks"} | ({"accumulate"} if o.get("accumulate") else set())
    elif op == "accum_f32":
        c |= {"copy" if o.get("copy") else "add", "grid_stride" if s["n"] // 4 > OPT_CAP else "one_trip"}
    elif op in ("adan", "adamw"):
        c.add("grid_stride" if s["n"] > OPT_CAP else "one_trip")
        c.add("clip" if o.get("clip", True) and o.get("max_norm", 1.0) > 0 else "no_clip")
        c.add("shadow" if o.get("shadow", True) else "no_shadow")
        if o.get("grad_scale", 1.0) != 1.0:
            c.add("grad_scale")
        if op == "adan":
            c.add("no_prox" if o.get("no_prox", True) else "prox")
        if o.get("wd", 0.0) > 0:
            c.add("wd")
    else:
        c.add("run")         # cast_f32_bf16, cast_bf16_f32, patchify, vit_assemble, transpose_batched, pooler_build
    return {f"{op}/{x}" for x in c}


_NORM4 = ["NCH=1", "NCH=2", "NCH=4", "NCH=8", "partial_block"]
_P = {
    "layernorm_fwd": _NORM4 + ["stats", "no_stats", "strided"],
    "layernorm_bwd": ["NCH=1", "NCH=2", "partial_block", "one_trip", "grid_stride", "dgamma", "no_dgamma", "dx", "no_dx", "no_add", "add", "add_alias",
                      "accumulate", "strided", "nan_workspace"],
    "rmsnorm_fwd": _NORM4 + ["rstd", "no_rstd", "strided"],
    "rmsnorm_fwd_q": ["NCH=1", "NCH=2", "NCH=4", "NCH=8", "partial_block", "y", "no_y"],
    "rmsnorm_bwd": _NORM4 + ["rstd", "recompute", "no_add", "add", "add_alias", "dy_alias"],
    "rmsnorm_bwd_q": ["NCH=1", "NCH=4", "NCH=8", "partial_block", "rstd", "recompute", "no_add", "add"],
    "rope": ["D=64", "D=128", "pos_ids", "pos_mod", "pos0", "inverse", "strided", "one_trip", "grid_stride"],
    "swiglu_fwd": ["one_trip", "grid_stride"],
    "swiglu_bwd": ["one_trip", "grid_stride", "alias"],
    "map": ["op0", "op1", "op2", "op3", "alias", "one_trip", "grid_stride"],
    "dropout": ["p0", "p", "strided"],
    "colsum": ["nsplit=1", "nsplit>1", "nsplit_cap", "accumulate", "strided"],
    "transpose": ["pad", "no_pad"],
    "transpose_batched": ["run"],
    "cast_f32_bf16": ["run"], "cast_bf16_f32": ["run"], "patchify": ["run"], "vit_assemble": ["run"],
    "gather_rows": ["one_trip", "multi_trip"], "scatter_rows": ["one_trip", "multi_trip"],
    "pooler_build": ["run"],
    "pooler_query_grad": ["dkv", "no_dkv", "accumulate"],
    "ce": ["idle_threads", "one_trip", "multi_trip", "no_grad", "inplace", "out_of_place", "strided"],
    "sqnorm": ["one_block", "blocks", "grid_stride", "accumulate"],
    "accum_f32": ["copy", "add", "one_trip", "grid_stride"],
    "adan": ["one_trip", "grid_stride", "clip", "no_clip", "shadow", "no_shadow", "grad_scale", "prox", "no_prox", "wd"],
    "adamw": ["one_trip", "grid_stride", "clip", "no_clip", "shadow", "no_shadow", "grad_scale", "wd"],
}
paths = {f"{op}/{x}" for op, xs in _P.items() for x in xs}

# ------------------------------------------------------------------------------------------------------------------------- cases
Case = namedtuple("Case", "op name shape opt")


def _c(_op, shape, **opt):
    name = ",".join(f"{k}={v}" for k, v in list(shape.items()) + list(opt.items()))
    return Case(_op, name, shape, opt)


def _build_cases():
    C = []
    for cols in (512, 1024, 2048, 4096):
        for i, rows in enumerate((1, 3, 4, 5, 9)):
            for stats in (True, False):
                C.append(_c("layernorm_fwd", dict(rows=rows, cols=cols), stats=stats, strided=bool((i + stats) % 2 or rows == 9)))
            C.append(_c("rmsnorm_fwd", dict(rows=rows, cols=cols), rstd=bool(i % 2), strided=bool(i % 2 == 0)))
            C.append(_c("rmsnorm_fwd_q", dict(rows=rows, cols=cols), y=bool(i % 2 == 0)))
            for rstd in (True, False):
                C.append(_c("rmsnorm_bwd", dict(rows=rows, cols=cols), rstd=rstd, add=(None, "separate", "alias")[(i + rstd) % 3], dy_alias=bool(i == 2 and rstd)))
        if cols != 1024:
            C.append(_c("rmsnorm_bwd_q", dict(rows=5, cols=cols), rstd=cols == 512, add="separate" if cols == 4096 else None))
    adds = (None, "separate", "alias")
    k = 0
    for cols in (512, 1024):
        for rows in (1, 3, 1024, 1025, 2057):
            for dgamma in (True, False):
                need_dx = not (dgamma and rows in (3, 1025))
                C.append(_c("layernorm_bwd", dict(rows=rows, cols=cols), dgamma=dgamma, accumulate=bool(dgamma and k // 2 % 2), need_dx=need_dx,
                            add=adds[k % 3] if need_dx else None, strided=bool(k % 4 < 2), nan_workspace=dgamma))
                k += 1
    C += [
        _c("rope", dict(rows=77, nheads=3, D=64), strided=True, pos_mod=30, pos0=7),
        _c("rope", dict(rows=77, nheads=1, D=128), strided=True, pos_mod=30, pos0=7, inverse=True),
        _c("rope", dict(rows=77, nheads=3, D=128), pos_ids=True, strided=True),
        _c("rope", dict(rows=77, nheads=1, D=64), pos_ids=True, inverse=True),
        _c("rope", dict(rows=4097, nheads=64, D=128), pos_mod=273),
        _c("swiglu_fwd", dict(rows=1, F=8)), _c("swiglu_fwd", dict(rows=301, F=11008)), _c("swiglu_fwd", dict(rows=1525, F=11008)),
        _c("swiglu_bwd", dict(rows=1, F=8), alias=True), _c("swiglu_bwd", dict(rows=301, F=11008)), _c("swiglu_bwd", dict(rows=301, F=11008), alias=True),
        _c("swiglu_bwd", dict(rows=1525, F=11008), alias=True),
    ]
    for op in range(4):
        C += [_c("map", dict(n=8), op=op, alias=bool(op % 2)), _c("map", dict(n=40008), op=op, alias=not op % 2)]
        C.append(_c("map", dict(n=16777232), op=op, alias=bool(op % 2)))
    C += [_c("dropout", dict(rows=37, cols=264), p=0.0, strided=True), _c("dropout", dict(rows=37, cols=264), p=0.05, strided=True),
          _c("dropout", dict(rows=300, cols=64), p=0.05)]
    for i, rows in enumerate((1, 255, 256, 257, 16385)):
        for j, cols in enumerate((1, 63, 64, 65, 1000)):
            C.append(_c("colsum", dict(rows=rows, cols=cols), accumulate=bool((i + j) % 2), strided=bool((i + j) % 3 != 1)))
    C += [_c("transpose", dict(rows=61, cols=70, rows_pad=72, extra=8)), _c("transpose", dict(rows=130, cols=65, rows_pad=130, extra=0)),
          _c("transpose", dict(rows=100, cols=200, rows_pad=192, extra=16)),
          _c("transpose_batched", dict(shapes=((70, 33), (64, 130), (129, 65), (5, 8)))),
          _c("cast_f32_bf16", dict(n=1025)), _c("cast_bf16_f32", dict(n=1025)),
          _c("patchify", dict(B=1, img=28, P=14, KP=640)),
          _c("vit_assemble", dict(B=2, NP=4, dim=8)), _c("vit_assemble", dict(B=2, NP=4, dim=1024))]
    for dim in (8, 4096):
        C += [_c("gather_rows", dict(n=11, src_rows=7, dim=dim)), _c("scatter_rows", dict(n=7, dst_rows=13, dim=dim))]
    for nq, ni, dim, B in (((64, 48, 32), (256, 256, 256), 1024, 2), ((2, 1, 3), (1, 4, 2), 8, 2)):
        C.append(_c("pooler_build", dict(nq=nq, ni=ni, dim=dim, B=B)))
        C += [_c("pooler_query_grad", dict(nq=nq, ni=ni, dim=dim, B=B), dkv=True, accumulate=False),
              _c("pooler_query_grad", dict(nq=nq, ni=ni, dim=dim, B=B), dkv=False, accumulate=True),
              _c("pooler_query_grad", dict(nq=nq, ni=ni, dim=dim, B=B), dkv=True, accumulate=True)]
    for V in (8, 2040, 2048, 2056, 32000):
        for n in (1, 77):
            C += [_c("ce", dict(n=n, V=V), grad=True, inplace=True, strided=True), _c("ce", dict(n=n, V=V), grad=False, strided=n == 1)]
        C.append(_c("ce", dict(n=77, V=V), grad=True, inplace=False, strided=True))
    C.append(_c("ce", dict(n=2, V=8), grad=True, inplace=True, strided=True))          # the smallest n at which 1/n and 1/(n-1) are both finite
    C += [_c("sqnorm", dict(n=n), accumulate=bool(i % 2)) for i, n in enumerate((1, 255, 257, 1048576 + 257))]
    C += [_c("sqnorm", dict(n=257), accumulate=True)]
    C += [_c("accum_f32", dict(n=n), copy=cp) for n in (4, 4194304 + 8) for cp in (True, False)]
    C += [
        _c("adan", dict(n=10007), no_prox=True, wd=0.0, clip=True, max_norm=1.0, grad_scale=1.0, shadow=True),
        _c("adan", dict(n=10007), no_prox=False, wd=0.02, clip=True, max_norm=1.0, grad_scale=0.25, shadow=True),
        _c("adan", dict(n=10007), no_prox=True, wd=0.02, clip=False, max_norm=1.0, grad_scale=1.0, shadow=False),
        _c("adan", dict(n=10007), no_prox=False, wd=0.0, clip=True, max_norm=0.0, grad_scale=0.25, shadow=True),
        _c("adan", dict(n=1048576 + 257), no_prox=True, wd=0.02, clip=True, max_norm=1.0, grad_scale=1.0, shadow=True),
        _c("adamw", dict(n=10007), wd=0.02, clip=True, max_norm=1.0, grad_scale=1.0, shadow=True),
        _c("adamw", dict(n=10007), wd=0.0, clip=False, max_norm=1.0, grad_scale=0.25, shadow=False),
        _c("adamw", dict(n=10007), wd=0.02, clip=True, max_norm=0.0, grad_scale=1.0, shadow=True),
        _c("adamw", dict(n=1048576 + 257), wd=0.02, clip=True, max_norm=1.0, grad_scale=0.25, shadow=True),
    ]
    return C


CASES = _build_cases()
CPU_MAX_ELEMS = 4_000_000          # cases above this many elements run on the GPU only


def case_elems(c):
    s = c.shape
    if "n" in s and "V" in s:
        return s["n"] * s["V"]
    if "n" in s and "dim" not in s:
        return s["n"]
    if c.op == "rope":
        return s["rows"] * s["nheads"] * s["D"]
    if "F" in s:
        return s["rows"] * s["F"] * 2
    if "rows" in s:
        return s["rows"] * s["cols"]
    return 1


def cases_of(op, cpu=False):
    return [c for c in CASES if c.op == op and (not cpu or case_elems(c) <= CPU_MAX_ELEMS)]


def seed_of(c):
    return zlib.crc32((c.op + ":" + c.name).encode())


# ------------------------------------------------------------------------------------------------------------------------- inputs (CPU tensors)
def edge_rows(x, shift):
    """float32 [rows, cols] in place: rows (r + shift) % 5 == 1 all zero, 2 constant (variance 0), 3 one outlier of 1e4 among 1e-2, 4 all |x|
    near 1e-20; only among the first 10 rows"""
    for r in range(min(x.shape[0], 10)):
        k = (r + shift) % 5
        if k == 1:
            x[r] = 0
        elif k == 2:
            x[r] = 0.75
        elif k == 3:
            x[r] *= 1e-2
            x[r, 7] = 1e4
        elif k == 4:
            x[r] *= 1e-20
    return x


def norm_inputs(c):
    """x, dy, gamma / w, beta, add (bf16), dgamma / dbeta prefill (fp32) of a norm case"""
    g = torch.Generator().manual_seed(seed_of(c))
    rows, cols = c.shape["rows"], c.shape["cols"]
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x = edge_rows(r(rows, cols) + 0.1, cols // 512).to(BF)
    return dict(x=x, dy=r(rows, cols).to(BF), gamma=(1 + r(cols, sc=0.3)).to(BF), beta=r(cols, sc=0.3).to(BF), add=r(rows, cols).to(BF),
                old=(r(cols, sc=rows ** 0.5), r(cols, sc=rows ** 0.5)))


SWIGLU_GATES = (0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4)


def swiglu_inputs(c):
    g = torch.Generator().manual_seed(seed_of(c))
    rows, F = c.shape["rows"], c.shape["F"]
    gu = torch.randn(rows, 2 * F, generator=g) * 2
    k = min(F, len(SWIGLU_GATES))
    gu[0, :k] = torch.tensor(SWIGLU_GATES[:k])                 # F = 8: the first eight; the wide cases: all ten
    if rows > 1:
        gu[rows - 1, F - k:F] = torch.tensor(SWIGLU_GATES[len(SWIGLU_GATES) - k:])
    return dict(gu=gu.to(BF), dact=torch.randn(rows, F, generator=g).to(BF))


def ce_inputs(c):
    """rows cycle through: random, all logits equal (loss = log V), one dominant logit with spread 60, random + 200; targets 0 and V - 1 on the
    first two rows"""
    g = torch.Generator().manual_seed(seed_of(c))
    n, V = c.shape["n"], c.shape["V"]
    x = torch.randn(n, V, generator=g) * 2
    kind0 = V // 8 % 4 if n == 1 else 0
    for r in range(n):
        k = (r + kind0) % 4
        if k == 1:
            x[r] = 1.5
        elif k == 2:
            x[r] = x[r].clamp(-3, 3) * 5 - 15
            x[r, (r * 7) % V] = 30.0
        elif k == 3:
            x[r] += 200
    t = torch.randint(0, V, (n,), generator=g)
    t[0] = V - 1 if n == 1 and V % 16 == 8 else 0
    if n > 1:
        t[1] = V - 1
    if n > 2:
        t[2] = (2 * 7) % V          # the dominant logit's own column on a spread-60 row
    return dict(x=x.to(BF), t=t.to(torch.int32))


OPT_LR, ADAN_BETAS, ADAMW_BETAS, OPT_EPS = 1e-3, (0.98, 0.92, 0.99), (0.9, 0.95), 1e-8


def opt_inputs(c):
    """p0 and four gradients, the second 100x larger, so that the clip at max_norm = 1 is off, on, off, off"""
    g = torch.Generator().manual_seed(seed_of(c))
    n = c.shape["n"]
    gs = c.opt.get("grad_scale", 1.0)
    # ||g_k|| * grad_scale = 0.3 at steps 1, 3, 4 (below max_norm = 1: not clipped) and 30 at step 2 (clipped)
    grads = [torch.randn(n, generator=g) * (0.3 / gs / n ** 0.5) * (100.0 if k == 1 else 1.0) for k in range(4)]
    return dict(p=torch.randn(n, generator=g), grads=grads)


def rope_inputs(c):
    g = torch.Generator().manual_seed(seed_of(c))
    rows, nheads, D = c.shape["rows"], c.shape["nheads"], c.shape["D"]
    npos = 320
    cos_t, sin_t = rope_tables(npos, D)
    if c.opt.get("pos_ids"):
        pos = torch.randint(0, npos - 1, (rows,), generator=g)            # non-monotone, with repeats
        pos[1], pos[2] = pos[0], pos[0]
    else:
        pos = torch.arange(rows) % c.opt["pos_mod"] + c.opt.get("pos0", 0)
    return dict(x=torch.randn(rows, nheads * D, generator=g).to(BF), cos=cos_t, sin=sin_t, pos=pos)


def map_inputs(c):
    g = torch.Generator().manual_seed(seed_of(c))
    n = c.shape["n"]
    return dict(a=(torch.randn(n, generator=g) * 3).to(BF), b=(torch.randn(n, generator=g) * 3).to(BF))


def mat_inputs(c, rows, cols, scale=1.0):
    g = torch.Generator().manual_seed(seed_of(c))
    return (torch.randn(rows, cols, generator=g) * scale).to(BF), torch.randn(cols, generator=g) * rows ** 0.5


def assemble_inputs(c):
    g = torch.Generator().manual_seed(seed_of(c))
    B, NP, dim = c.shape["B"], c.shape["NP"], c.shape["dim"]
    r = lambda *s: torch.randn(*s, generator=g).to(BF)
    return dict(patch=r(B * NP, dim), cls=r(dim), pos=r(NP + 1, dim))


def qgrad_inputs(c):
    g = torch.Generator().manual_seed(seed_of(c))
    s = c.shape
    NQ, KV = sum(s["nq"]), sum(s["nq"]) + sum(s["ni"])
    return dict(dt0=torch.randn(s["B"] * NQ, s["dim"], generator=g).to(BF), dkv=torch.randn(s["B"] * KV, s["dim"], generator=g).to(BF),
                old=torch.randn(NQ, s["dim"], generator=g))


def sqnorm_inputs(c):
    g = torch.Generator().manual_seed(seed_of(c))
    return dict(g=torch.randn(c.shape["n"], generator=g), old=torch.rand(1, generator=g) * c.shape["n"])


def opt_args(c):
    o = c.opt
    kw = dict(lr=OPT_LR, eps=OPT_EPS, wd=o["wd"], clip=o["clip"], max_norm=o["max_norm"], grad_scale=o["grad_scale"])
    if c.op == "adan":
        kw.update(betas=ADAN_BETAS, no_prox=o["no_prox"])
    else:
        kw.update(betas=ADAMW_BETAS)
    return kw


def opt_state0(c, p):
    z = lambda: torch.zeros_like(p)
    return dict(p=p.clone(), m=z(), v=z(), n=z(), pre=None) if c.op == "adan" else dict(p=p.clone(), m=z(), v=z())


def ln_stats_f32(inp):
    """the saved statistics a backward case is handed: the float64 ones rounded to fp32"""
    r = ref_layernorm_fwd(inp["x"], inp["gamma"], inp["beta"], 1e-5)
    return r["mean"].want.float(), r["rstd"].want.float()


def emulate(c, mut=None):
    """-> [(kind, what, got, Ref)] of the float32 emulation (with defect `mut`) against the float64 reference on case c (CPU)"""
    op, s, o = c.op, c.shape, c.opt
    out = []

    def add(kind, got, ref, names=None):
        for k in names or ref:
            out.append((kind[k] if isinstance(kind, dict) else kind, k, got[k], ref[k]))

    if op == "layernorm_fwd":
        i = norm_inputs(c)
        add(dict(y="ln_y", mean="ln_stats", rstd="ln_stats"), emu_layernorm_fwd(i["x"], i["gamma"], i["beta"], 1e-5, mut), ref_layernorm_fwd(i["x"], i["gamma"], i["beta"], 1e-5))
    elif op == "layernorm_bwd":
        i = norm_inputs(c)
        mean, rstd = ln_stats_f32(i)
        kw = dict(add=i["add"] if o["add"] else None, old=i["old"] if o["accumulate"] else None, need_dx=o["need_dx"], need_dg=o["dgamma"])
        add(dict(dx="ln_dx", dgamma="ln_dgamma", dbeta="ln_dgamma"), emu_layernorm_bwd(i["dy"], i["x"], i["gamma"], mean, rstd, mut=mut, **kw),
            ref_layernorm_bwd(i["dy"], i["x"], i["gamma"], mean, rstd, **kw))
    elif op == "rmsnorm_fwd":
        i = norm_inputs(c)
        add(dict(y="rms_y", rstd="rms_rstd"), emu_rmsnorm_fwd(i["x"], i["gamma"], 1e-5, mut), ref_rmsnorm_fwd(i["x"], i["gamma"], 1e-5))
    elif op == "rmsnorm_bwd":
        i = norm_inputs(c)
        rstd = ref_rmsnorm_fwd(i["x"], i["gamma"], 1e-5)["rstd"].want.float() if o["rstd"] else None
        kw = dict(rstd=rstd, add=i["add"] if o["add"] else None)
        add("rms_dx", emu_rmsnorm_bwd(i["dy"], i["x"], i["gamma"], mut=mut, **kw), ref_rmsnorm_bwd(i["dy"], i["x"], i["gamma"], **kw))
    elif op == "rope":
        i = rope_inputs(c)
        a = (i["x"], i["cos"], i["sin"], i["pos"], s["nheads"], s["D"], bool(o.get("inverse")))
        add("rope", emu_rope(*a, mut=mut), ref_rope(*a))
    elif op == "swiglu_fwd":
        i = swiglu_inputs(c)
        add("swiglu_act", emu_swiglu_fwd(i["gu"], s["F"], mut), ref_swiglu_fwd(i["gu"], s["F"]))
    elif op == "swiglu_bwd":
        i = swiglu_inputs(c)
        add("swiglu_dgu", emu_swiglu_bwd(i["dact"], i["gu"], s["F"], mut), ref_swiglu_bwd(i["dact"], i["gu"], s["F"]))
    elif op == "map":
        i = map_inputs(c)
        add("map", emu_map(o["op"], i["a"], i["b"], mut), ref_map(o["op"], i["a"], i["b"]))
    elif op == "vit_assemble":
        i = assemble_inputs(c)
        add("assemble", emu_assemble(i["patch"], i["cls"], i["pos"], s["B"], s["NP"]), ref_assemble(i["patch"], i["cls"], i["pos"], s["B"], s["NP"]))
    elif op == "colsum":
        x, old = mat_inputs(c, s["rows"], s["cols"])
        old = old if o["accumulate"] else None
        add("colsum", emu_colsum(x, old, mut), ref_colsum(x, old))
    elif op == "sqnorm":
        i = sqnorm_inputs(c)
        old = i["old"] if o["accumulate"] else None
        add("sqnorm", emu_sqnorm(i["g"], old, mut), ref_sqnorm(i["g"], old))
    elif op == "pooler_query_grad":
        i = qgrad_inputs(c)
        a = (i["dt0"], i["dkv"] if o["dkv"] else None, s["B"], s["nq"], s["ni"], i["old"] if o["accumulate"] else None)
        add("qgrad", emu_query_grad(*a, mut=mut), ref_query_grad(*a))
    elif op == "ce":
        i = ce_inputs(c)
        names = ("row_loss", "loss", "grad") if o["grad"] else ("row_loss", "loss")
        add(dict(row_loss="ce_loss", loss="ce_loss", grad="ce_grad"), emu_ce(i["x"], i["t"], mut), ref_ce(i["x"], i["t"]), names)
    elif op in ("adan", "adamw"):
        i = opt_inputs(c)
        st = opt_state0(c, i["p"])
        emu, ref = (emu_adan, ref_adan) if op == "adan" else (emu_adamw, ref_adamw)
        for k, g in enumerate(i["grads"]):
            r = ref(st, g, k + 1, **opt_args(c))                     # one step from the state the emulation is in
            new = emu(st, g, k + 1, mut=mut, **opt_args(c))
            for name in r:
                out.append((op, f"step {k + 1} {name}", new[name], r[name]))
            st = {name: new[name] for name in st}
    return out


EMULATED = ("layernorm_fwd", "layernorm_bwd", "rmsnorm_fwd", "rmsnorm_bwd", "rope", "swiglu_fwd", "swiglu_bwd", "map", "vit_assemble", "colsum",
            "sqnorm", "pooler_query_grad", "ce", "adan", "adamw")

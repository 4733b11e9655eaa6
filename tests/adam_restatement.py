"""The Adam step of e2emv_adam_step / E.Adam restated in fp64 from fp32 inputs, and the bars a fp32 implementation is held to.

With t = step + 1 (torch.optim.Adam without weight decay or amsgrad, after clip_grad_value_):

    g  = clamp(g, -c, c)                       (c = float32(clip): a selection, exact)
    m' = m + (g - m)(1 - beta1)
    v' = beta2 v + (1 - beta2) g^2
    p' = p - (lr / (1 - beta1^t)) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)

Bars, u = 2^-24 (the relative error of one fp32 rounding), g the clipped gradient, m and v the moments BEFORE the step:

    |dm| <= 4u max(|m|, |g|)        three roundings of quantities no larger than max(|m|, |g|), one to spare
    |dv| <= 4u max(v, g^2)          likewise
    |dp| <= 2u |p'| + 16u |update|  the update inherits 1u from m' and 2u from sqrt(v') and takes five roundings of its own
                                    (step size, division by the bias correction, + eps, m / denom, the product) - 8u, doubled;
                                    the final subtraction is one rounding of p' - 1u, doubled

Each step is compared from the implementation's OWN previous state (teacher-forced), so errors do not accumulate into the bars.
"""
import torch

U = 2.0 ** -24
SCALES = (1e-6, 1e-3, 1.0, 50.0)
CLIP = 0.1


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, clip=None):
    """One step in fp64.  p, g, m, v: tensors of any float dtype (taken as they are, usually fp32); step: the number of steps
    taken so far.  Returns {"p", "m", "v", "g" (clipped), "update", "m_old", "v_old"}, all float64, on the CPU."""
    p, g, m, v = (x.detach().to("cpu", torch.float64) for x in (p, g, m, v))
    if clip is not None:
        c = float(torch.tensor(clip, dtype=torch.float32))
        g = g.clamp(-c, c)
    t = float(step) + 1.0
    m2 = m + (g - m) * (1.0 - beta1)
    v2 = beta2 * v + (1.0 - beta2) * g * g
    update = (lr / (1.0 - beta1 ** t)) * m2 / (v2.sqrt() / (1.0 - beta2 ** t) ** 0.5 + eps)
    return {"p": p - update, "m": m2, "v": v2, "g": g, "update": update, "m_old": m, "v_old": v}


def bars(ref):
    g = ref["g"]
    bm = 4 * U * torch.maximum(ref["m_old"].abs(), g.abs())
    bv = 4 * U * torch.maximum(ref["v_old"], g * g)
    bp = 2 * U * ref["p"].abs() + 16 * U * ref["update"].abs()
    return bm, bv, bp


def ratios(ref, p, m, v, keep=None):
    """max |error| / bar of (m, v, p) over the elements of `keep` (default: all); 0 / 0 counts as 0, x / 0 as inf."""
    out = []
    for got, key, bar in zip((m, v, p), ("m", "v", "p"), bars(ref)):
        err = (got.detach().to("cpu", torch.float64) - ref[key]).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bar)
        r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
        if keep is not None:
            r = r[keep]
        out.append(float(r.max()) if r.numel() else 0.0)
    return tuple(out)


def make_grad(shape, seed, scale):
    """A deterministic fp32 gradient of one scale with exact zeros and entries exactly at +-float32(CLIP) sprinkled in."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(shape, generator=gen, dtype=torch.float32) * scale
    flat = g.reshape(-1)
    n = flat.numel()
    if n >= 3:
        idx = torch.randperm(n, generator=gen)
        k = max(1, n // 7)
        flat[idx[:k]] = 0.0
        flat[idx[k:k + max(1, n // 11)]] = CLIP
        flat[idx[k + max(1, n // 11):k + 2 * max(1, n // 11)]] = -CLIP
    return g

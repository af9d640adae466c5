"""Which roundings torch's device kernels make in one step of torch.optim.Adam(foreach=False, fused=False), measured on the device the
native step (csrc/adam.hip) has to agree with.  Every op of _single_tensor_adam is run on its own with torch, and its float32 result is
compared, element by element, with candidate evaluations built from float64 arithmetic:

    fused      f32(a * b + c)   with the product exact in float64 (two float32 factors) -- one rounding, up to a double rounding in ~2^-29 of cases
    unfused    f32(f32(a * b) + c)

    python tools/adam_convention.py [--n 4000000] [--out profiles/optim_adam_convention.txt]

Prints, per op, the fraction of elements each candidate reproduces bit for bit, then how many elements of a whole native step differ
from torch's.  Needs a HIP device."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "lidar-gs_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    f32 = lambda x: torch.tensor(x, dtype=torch.float64).float().double().item()      # a Python double rounded to float32
    same = lambda x, y: float(((x.view(torch.int32) == y.view(torch.int32)) | (x.isnan() & y.isnan())).double().mean())
    gen = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda: torch.randn(a.n, device="cuda", generator=gen)
    p, g, m, v = rnd(), 0.1 * rnd() * rnd().abs(), 0.05 * rnd(), (0.05 * rnd()) ** 2
    pd, gd, md, vd = p.double(), g.double(), m.double(), v.double()
    beta1, beta2, eps, lr, step = 0.9, 0.999, 1e-15, 7.5e-3, 7
    say(f"device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, n = {a.n}, beta1 {beta1} beta2 {beta2} eps {eps} lr {lr} step {step}")

    w1 = f32(1 - beta1)
    m_t = m.clone().lerp_(g, 1 - beta1)
    d32 = (g - m).double()
    say(f"lerp_(grad, 1 - beta1)        fused fma(w, g - m, m) {same(m_t, (w1 * d32 + md).float()):.6f}   unfused m + f32(w * (g - m)) {same(m_t, ((w1 * d32).float().double() + md).float()):.6f}")

    b2, w2 = f32(beta2), f32(1 - beta2)
    v1 = v.clone().mul_(beta2)
    say(f"mul_(beta2)                   v * f32(beta2) {same(v1, (vd * b2).float()):.6f}")
    v_t = v1.clone().addcmul_(g, g, value=1 - beta2)
    gg = (g * g).double()
    say(f"addcmul_(g, g, value=1-beta2) fused fma(w, f32(g * g), v) {same(v_t, (w2 * gg + v1.double()).float()):.6f}   "
        f"unfused v + f32(w * f32(g * g)) {same(v_t, ((w2 * gg).float().double() + v1.double()).float()):.6f}   "
        f"fma(f32(w * g), g, v) {same(v_t, ((w2 * gd).float().double() * gd + v1.double()).float()):.6f}")

    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    bc2_sqrt = bc2 ** 0.5
    s_t = v_t.sqrt()
    say(f"sqrt()                        correctly rounded {same(s_t, v_t.double().sqrt().float()):.6f}")
    q_t = s_t / bc2_sqrt
    sd = s_t.double()
    say(f"/ bias_correction2_sqrt       x * f32(1 / s) {same(q_t, (sd * f32(1.0 / bc2_sqrt)).float()):.6f}   x * f32(1 / f32(s)) {same(q_t, (sd * f32(1.0 / f32(bc2_sqrt))).float()):.6f}   "
        f"ieee x / f32(s) {same(q_t, (sd / f32(bc2_sqrt)).float()):.6f}   f32(x / s in f64) {same(q_t, (sd / bc2_sqrt).float()):.6f}")
    den_t = q_t.clone().add_(eps)
    say(f"add_(eps)                     x + f32(eps) {same(den_t, (q_t.double() + f32(eps)).float()):.6f}")
    alpha = f32(-(lr / bc1))
    r_t = m_t / den_t
    say(f"tensor / tensor               correctly rounded {same(r_t, (m_t.double() / den_t.double()).float()):.6f}")
    p_t = p.clone().addcdiv_(m_t, den_t, value=-(lr / bc1))
    rd = r_t.double()
    say(f"addcdiv_(m, denom, value)     fused fma(a, f32(m / d), p) {same(p_t, (alpha * rd + pd).float()):.6f}   unfused p + f32(a * f32(m / d)) {same(p_t, ((alpha * rd).float().double() + pd).float()):.6f}   "
        f"p + f32(f32(a * m) / d) {same(p_t, (((alpha * m_t.double()).float().double() / den_t.double()).float().double() + pd).float()):.6f}")

    # the whole step: torch's optimizer against the native one, from the same state
    from torch import nn
    import build_hip
    build_hip.build()
    from lidargs_optim import Adam

    def run(cls, **kw):
        q = nn.Parameter(p.clone())
        opt = cls([q], lr=lr, betas=(beta1, beta2), eps=eps, **kw)
        q.grad = g.clone()
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        opt.step()
        torch.cuda.synchronize()
        return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]

    ref = run(torch.optim.Adam, foreach=False, fused=False)
    say(f"op-by-op chain above == torch.optim.Adam(foreach=False): param {same(ref[0], p_t):.6f} exp_avg {same(ref[1], m_t):.6f} exp_avg_sq {same(ref[2], v_t):.6f}")
    ours = run(Adam)
    diff = [int((x.view(torch.int32) != y.view(torch.int32)).sum()) for x, y in zip(ours, ref)]
    say(f"native step vs torch.optim.Adam(foreach=False): elements differing in bits of {a.n}: param {diff[0]}, exp_avg {diff[1]}, exp_avg_sq {diff[2]}")
    for name, kw in (("foreach=True", dict(foreach=True)),):
        oth = run(torch.optim.Adam, **kw)
        diff = [int((x.view(torch.int32) != y.view(torch.int32)).sum()) for x, y in zip(oth, ref)]
        say(f"torch {name} vs torch foreach=False: param {diff[0]}, exp_avg {diff[1]}, exp_avg_sq {diff[2]}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

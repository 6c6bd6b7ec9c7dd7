"""PAM attention probe (gd_pam_attn_stats / _received / _rows), kernel level: HIP-event medians at B = 1, N = 65 536, r = 23,
S = 64, alternated in one process with gd_pam_f32_fwd at C = 184 on the same q / k as the yardstick (the query sweep does
that kernel's S product and exp and none of its P V).
    python tools/pam_probe_bench.py --out profiles/r11_pam_probe.txt
TF of the S product: 2 N^2 r B per sweep (the rows kernel sweeps S queries twice: 4 N S r B)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gan_danet_amd import kern as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--tile", type=int, default=256)
ap.add_argument("--channels", type=int, default=184)
ap.add_argument("--points", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda")
B, C, N, S = a.batch, a.channels, a.tile * a.tile, a.points
r = C // 8
assert N % 256 == 0

g = torch.Generator(device=dev).manual_seed(0)
q = torch.randn(B, r, N, device=dev, generator=g) * 0.5
k = torch.randn(B, r, N, device=dev, generator=g) * 0.5
v, x = (torch.randn(B, C, N, device=dev, generator=g) for _ in range(2))
gamma = torch.tensor([0.7], device=dev)
out, o = torch.empty_like(x), torch.empty_like(x)
lse, ent, peak, rec = (torch.empty(B, N, device=dev) for _ in range(4))
lse_y = torch.empty(B, N, device=dev)
idx = torch.randperm(N, device=dev, generator=g)[:S].to(torch.int32)
rows = torch.empty(B, S, N, device=dev)

fns = {
    "pam_attn_stats": (lambda: K.pam_attn_stats(q, k, B, N, N, r, lse, ent, peak), 2.0 * N * N * r * B),
    "pam_attn_received": (lambda: K.pam_attn_received(q, k, lse, B, N, N, r, rec), 2.0 * N * N * r * B),
    "pam_attn_rows": (lambda: K.pam_attn_rows(q, k, idx, B, N, N, r, rows), 4.0 * N * S * r * B),
    "pam_f32_fwd (yardstick)": (lambda: K.pam_f32_fwd(q, k, v, B, N, N, C, r, gamma, x, out, o, lse_y), 2.0 * N * N * r * B),
}
times = {n: [] for n in fns}
for it in range(a.warmup + a.reps):              # alternated: every round times each kernel once
    for n, (fn, _) in fns.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[n].append(e0.elapsed_time(e1))

lines = [json.dumps(dict(device=torch.cuda.get_device_name(0), B=B, N=N, r=r, S=S, C_yardstick=C, reps=a.reps))]
yard = statistics.median(times["pam_f32_fwd (yardstick)"])
for n, (_, work) in fns.items():
    t = statistics.median(times[n])
    lines.append(json.dumps(dict(kernel=n, ms=round(t, 3), min_ms=round(min(times[n]), 3), max_ms=round(max(times[n]), 3),
                                 s_product_tflops=round(work / t * 1e-9, 2), ratio_to_yardstick=round(t / yard, 4))))
lines.append(json.dumps(dict(check="sum received / N", value=(rec.double().sum() / (B * N)).item(),
                             lse_equal_to_yardstick=bool(torch.equal(lse, lse_y)))))
print("\n".join(lines), flush=True)
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")

"""The Perceiver's attention core -- what lies between to_q / to_kv and to_out in perceiver_lang_io.py:102-145 -- three ways, at the
three shapes ManiGaussian runs (conf/method/ManiGaussian_BC.yaml:22-40), B = 1 and 2, fp32:
  ours       manigaussian_amd.attention.fused_attention_kv on q [B,Nq,H 64] and the to_kv output [B,Nk,2 H 64] (csrc/mgs_attention.hip)
  torch_seq  the reference's operations written with torch calls: the three rearranges, einsum * scale, softmax, dropout, einsum,
             rearrange back (what the reference executes; its text is not here)
  sdpa_*     torch.nn.functional.scaled_dot_product_attention on the rearranged views, once per backend this torch offers for
             fp32 (a backend that refuses the call is reported as unavailable with its message)
in training mode (dropout as the table below) and eval mode (no dropout), forward alone and forward + backward.  Variants are
alternated call by call in one process after warm-up; times are hipEvent medians around each call.  Peak memory: the largest
torch.cuda.max_memory_allocated() above the inputs during one forward + backward.  Achieved TFLOP/s: the algorithmic operations
(forward 4 B H Nq Nk 64, backward 10 B H Nq Nk 64: two and five matrix products) over the median, beside the 157.3 TFLOP/s fp32
matrix peak of an MI355X; ours recomputes the scores in both backward kernels (seven products), which this figure does not credit.
Prints one JSON line and writes it to --out (default profiles/attention_bench.json).  BA_STEPS: timed steps (30).
BA_ONLY=ours|torch_seq: that variant's training forward + backward only at B = 1, untimed (for rocprofv3 --kernel-trace --stats).
Needs a HIP device: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from manigaussian_amd import _lib  # noqa: E402
from manigaussian_amd.attention import fused_attention_kv  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.json"))
args = ap.parse_args()
STEPS = int(os.environ.get("BA_STEPS", "30"))
WARM = 5
PEAK_TFLOPS = 157.3
SHAPES = {  # name: heads, queries, keys, dropout in training
    "encoder_cross": (1, 2048, 8077, 0.1),
    "latent_self": (8, 2048, 2048, 0.1),
    "decoder_cross": (1, 8077, 2048, 0.0),
}
assert torch.cuda.is_available(), "bench_attention.py needs a HIP device"
dev = torch.device("cuda:0")


def split_heads(t, H):  # rearrange 'b n (h d) -> (b h) n d'
    B, N, _ = t.shape
    return t.reshape(B, N, H, 64).permute(0, 2, 1, 3).reshape(B * H, N, 64)


def torch_seq(q, kv, H, p):
    B, Nq, _ = q.shape
    k, v = kv.chunk(2, dim=-1)
    q, k, v = split_heads(q, H), split_heads(k, H), split_heads(v, H)
    sim = torch.einsum("bid,bjd->bij", q, k) * 64 ** -0.5
    attn = F.dropout(sim.softmax(dim=-1), p, training=p > 0)
    out = torch.einsum("bij,bjd->bid", attn, v)
    return out.reshape(B, H, Nq, 64).permute(0, 2, 1, 3).reshape(B, Nq, H * 64)


def sdpa(backend):
    from torch.nn.attention import sdpa_kernel

    def run(q, kv, H, p):
        B, Nq, _ = q.shape
        k, v = kv.chunk(2, dim=-1)
        q, k, v = (t.reshape(B, -1, H, 64).transpose(1, 2) for t in (q, k, v))
        with sdpa_kernel(backend):
            out = F.scaled_dot_product_attention(q, k, v, dropout_p=p)
        return out.transpose(1, 2).reshape(B, Nq, H * 64)
    return run


class Ours:
    def __init__(self):
        self.state = torch.tensor([1234, 0], dtype=torch.int64, device=dev)

    def __call__(self, q, kv, H, p):
        rng = None
        if p > 0:
            rng = self.state.clone()
            self.state[1:].add_(1)
        return fused_attention_kv(q, kv, H, dropout_p=p, rng_state=rng)


def variants():
    v = {"ours": Ours(), "torch_seq": torch_seq}
    try:
        from torch.nn.attention import SDPBackend
        for name in ("MATH", "EFFICIENT_ATTENTION", "FLASH_ATTENTION"):
            if hasattr(SDPBackend, name):
                v["sdpa_" + name.lower()] = sdpa(getattr(SDPBackend, name))
    except ImportError as e:
        print("torch.nn.attention is not available:", e)
    return v


def timed(fns, steps):
    ev = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for k, lst in ev.items():
        t = sorted(a.elapsed_time(b) for a, b in lst)
        out[k] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1]}
    return out


def bench(name, B):
    H, Nq, Nk, p_train = SHAPES[name]
    g = torch.Generator().manual_seed(7)
    q0 = torch.randn(B, Nq, H * 64, generator=g).to(dev)
    kv0 = torch.randn(B, Nk, 2 * H * 64, generator=g).to(dev)
    go = torch.randn(B, Nq, H * 64, generator=g).to(dev)
    q, kv = q0.clone().requires_grad_(True), kv0.clone().requires_grad_(True)
    fl_f, fl_b = 4.0 * B * H * Nq * Nk * 64, 10.0 * B * H * Nq * Nk * 64
    res = {"shape": dict(B=B, H=H, Nq=Nq, Nk=Nk, dropout_train=p_train), "flop_forward": fl_f, "flop_backward": fl_b}
    vs = variants()
    # which variants run here at all, and do they agree (p = 0)
    ref = torch_seq(q0, kv0, H, 0.0)
    usable = {}
    for k, fn in vs.items():
        try:
            out = fn(q, kv, H, 0.0)
            out.backward(go)
            q.grad = kv.grad = None
            torch.cuda.synchronize()
            usable[k] = fn
            res.setdefault("max_abs_diff_to_torch_seq", {})[k] = (out.detach() - ref).abs().max().item()
        except RuntimeError as e:
            res.setdefault("unavailable", {})[k] = str(e).strip().splitlines()[0][:300]
    for mode, p in (("train", p_train), ("eval", 0.0)):
        def fwd(fn):
            if mode == "eval":
                with torch.no_grad():
                    return fn(q0, kv0, H, p)
            return fn(q, kv, H, p)

        def fwd_bwd(fn):
            fn(q, kv, H, p).backward(go)
            q.grad = kv.grad = None

        for what, call in (("forward", fwd), ("forward_backward", fwd_bwd)):
            fns = {k: (lambda fn=fn: call(fn)) for k, fn in usable.items()}
            for _ in range(WARM):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
            t = timed(fns, STEPS)
            fl = fl_f if what == "forward" else fl_f + fl_b
            for k in t:
                tf = fl / (t[k]["median_ms"] * 1e-3) / 1e12
                t[k]["algorithmic_TFLOPs"] = tf
                t[k]["of_fp32_matrix_peak_157.3"] = tf / PEAK_TFLOPS
            res[f"{mode}/{what}"] = t
        mem = {}
        for k, fn in usable.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fwd_bwd(fn)
            torch.cuda.synchronize()
            mem[k] = torch.cuda.max_memory_allocated() - base
        res[f"{mode}/peak_bytes_forward_backward"] = mem
    return res


only = os.environ.get("BA_ONLY")
if only:  # profiling runs (rocprofv3 --kernel-trace --stats): one variant alone, eager
    fn = {"ours": Ours(), "torch_seq": torch_seq}[only]
    for name, (H, Nq, Nk, p) in SHAPES.items():
        q = torch.randn(1, Nq, H * 64, device=dev, requires_grad=True)
        kv = torch.randn(1, Nk, 2 * H * 64, device=dev, requires_grad=True)
        go = torch.randn(1, Nq, H * 64, device=dev)
        for _ in range(STEPS):
            fn(q, kv, H, p).backward(go)
            q.grad = kv.grad = None
    torch.cuda.synchronize()
    sys.exit(0)

res = {"steps": STEPS, "mgs_build_id": _lib.build_id(), "torch": torch.__version__,
       "note": "the attention core on q and the to_kv output (projections excluded in every variant); device times are hipEvent "
               "medians around each call, variants alternated call by call in one process; TFLOP/s are algorithmic operations "
               "over the median; peak bytes are above the inputs, during one forward + backward."}
for name in SHAPES:
    for B in (1, 2):
        res[f"{name}/B{B}"] = bench(name, B)
line = json.dumps(res)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(json.dumps(res, indent=1) + "\n")

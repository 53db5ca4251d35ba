"""Two builds of libmgsplat.so side by side on the kernels whose selects tests/test_nonfinite.py's findings changed (csrc/mgs_mlp.hip,
mgs_regress.hip, mgs_deform.hip, mgs_optim.hip, mgs_spatial_softmax.hip, mgs_dense.hip, mgs_volume.hip, mgs_narrow.hip, mgs_loss.hip): the bits of their outputs over the existing
case tables, and their times at ManiGaussian's sizes.

  python scripts/bench_nonfinite_ab.py --lib PATH --label NAME --out FILE

loads the library at PATH (default: the package's own) and writes one JSON row:
  hashes   per op, the SHA-256 of every output of every case of the op's table (tests/*_cases.py), in table order.  Finite inputs:
           two builds that compute the same bits -- the sign of a zero included -- give the same hash;
  times_us per kernel path, min / median / max over ROUNDS rounds of the mean of enough back-to-back calls between two device
           events to fill WINDOW seconds, after warm-up.
One process per build (a process holds one library); run the parent's build twice and this one once in one session and compare: a
difference counts only beyond the spread of the parent's two runs.  profiles/nonfinite_ab.json holds such a session's three rows.
Needs a HIP device: there is no CPU path."""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--label", default="this")
ap.add_argument("--out", required=True)
ap.add_argument("--no-times", action="store_true")
args = ap.parse_args()

from manigaussian_amd import _lib  # noqa: E402
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
assert torch.cuda.is_available(), "bench_nonfinite_ab.py needs a HIP device"
dev = torch.device("cuda:0")
ROUNDS, WINDOW = 7, 0.1


def mod(name):
    return importlib.import_module("manigaussian_amd." + name)


class Hash:
    def __init__(self):
        self.h, self.n = hashlib.sha256(), 0

    def add(self, *tensors):
        for t in tensors:
            if t is not None:
                self.h.update(t.detach().contiguous().cpu().numpy().tobytes())
                self.n += t.numel()

    def done(self):
        return {"sha256": self.h.hexdigest(), "elements": self.n}


def hashes():
    import dense_conv_cases as dc
    import embed_cases as ec
    import lamb_cases as lac
    import spatial_softmax_cases as ssc
    out = {}
    dfm, h = mod("deform"), Hash()
    for M in ec.MLP_M:
        for hidden in ec.MLP_HIDDEN:
            d = {k: v.to(dev) for k, v in ec.mlp_inputs(M, hidden).items()}
            a, xb = dfm._relu_bias(d["act"], d["bias"])
            h.add(a, xb)
            for res in (d["g_res"], None):
                cs = torch.zeros(hidden, device=dev)
                h.add(dfm._relu_backward(d["g_pre"].clone(), d["act"], res, cs))   # (the column sums are float atomics: not hashed)
    out["mlp"] = h.done()
    h = Hash()
    for N in ec.POINT_N:
        if N == 0:
            continue
        delta, xyz, rot, cot = ec.apply_inputs(N)
        delta = delta.to(dev).requires_grad_(True)
        nx, nr = dfm.deform_apply(delta, xyz.to(dev), rot.to(dev))
        torch.autograd.backward([nx, nr], [c.to(dev) for c in cot])
        h.add(nx, nr, delta.grad)
    out["deform_apply"] = h.done()
    h = Hash()
    for N in ec.POINT_N:
        if N == 0:
            continue
        raw, xyz_in, cot = ec.epilogue_inputs(N)
        raw, xyz_in = raw.to(dev).requires_grad_(True), xyz_in.to(dev).requires_grad_(True)
        o = mod("regressor").gaussian_epilogue(raw, xyz_in)
        torch.autograd.backward([o[k] for k in ec.EPILOGUE_OUTPUTS], [cot[k].to(dev) for k in ec.EPILOGUE_OUTPUTS])
        h.add(*[o[k] for k in ec.EPILOGUE_OUTPUTS], raw.grad, xyz_in.grad)
    out["gaussian_epilogue"] = h.done()
    h = Hash()
    for case in lac.CASES:
        inp = lac.make_inputs(case)
        ps = [t.to(dev).requires_grad_(True) for t in inp["params"]]
        groups = [dict(params=[ps[i] for i in g["idx"]], lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
                  for g in inp["groups"]]
        opt = mod("optim").FusedLamb(groups, adam=inp["adam"])
        for k in range(inp["K"]):
            for p, g in zip(ps, lac.gradients(inp, k)):
                p.grad = None if g is None else g.to(dev)
            opt.step()
            for p in ps:
                st = opt.state.get(p)
                if st:
                    h.add(st["weight_norm"], st["adam_norm"], st["trust_ratio"])
        for p in ps:
            st = opt.state.get(p)
            h.add(p, *([st["exp_avg"], st["exp_avg_sq"]] if st else []))
    out["fused_lamb"] = h.done()
    h = Hash()
    for case in ssc.CASES:
        for slices in (0, 1, 3):
            x, g_k, g_m = ssc.make_inputs(case)
            x = x.to(dev).requires_grad_(True)
            kp, mx = mod("spatial_softmax")._spatial_softmax3d(x, ssc.TEMPERATURE, slices=slices)
            torch.autograd.backward([kp, mx], [g_k.to(dev), g_m.to(dev)])
            h.add(kp, mx, x.grad)
    out["spatial_softmax"] = h.done()
    h = Hash()
    for case in dc.ALL:
        if case.startswith("long_sum"):
            continue
        t = dc.make_inputs(case)
        x, w = t["x"].to(dev).requires_grad_(True), t["w"].to(dev).requires_grad_(True)
        b = None if t["b"] is None else t["b"].to(dev).requires_grad_(True)
        y = mod("dense").dense_conv3d(x, w, b, dc.slope_of(case))
        y.backward(t["g"].to(dev))
        h.add(y, x.grad, w.grad, None if b is None else b.grad)
    out["dense"] = h.done()
    import volume_cases as vc
    h = Hash()
    for case in vc.CASES:
        _, scale, pad = vc.CASES[case]
        sources = [t.detach().requires_grad_(True) for t in vc.make_sources(case, dev)]
        o = mod("volume").resample_pad(sources, scale, pad)
        o.backward(vc.make_upstream(case, dev))
        h.add(o, *[t.grad for t in sources])
    out["resample_pad"] = h.done()
    import narrow_conv_cases as nc
    h = Hash()
    for case in nc.ALL:
        if case.startswith("long_sum"):
            continue
        t = nc.make_inputs(case)
        x, w = t["x"].to(dev).requires_grad_(True), t["w"].to(dev).requires_grad_(True)
        b = None if t["b"] is None else t["b"].to(dev).requires_grad_(True)
        y = mod("narrow").narrow_conv3d(x, w, b, nc.mode_of(case))
        y.backward(t["g"].to(dev))
        h.add(y, x.grad, w.grad, None if b is None else b.grad)
    out["narrow"] = h.done()
    import loss_cases as lc
    h = Hash()
    for case in lc.CASES:
        c = lc.CASES[case]
        inp, _ = lc.make_inputs(case)
        color, feature = inp["color"].to(dev).requires_grad_(True), inp["feature"].to(dev).requires_grad_(True)
        loss, terms = mod("losses").rendering_loss(color, lc.lay_out(inp["gt_rgb"], c["layout"][0]).to(dev), feature,
                                                   lc.lay_out(inp["gt_embed"], c["layout"][1]).to(dev), weights=c["weights"], embed_loss_fn=c["fn"])
        loss.backward()
        h.add(loss, color.grad, feature.grad, *[terms[k] for k in sorted(terms)])
    out["rendering_loss"] = h.done()
    return out


def timed(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / calls


def measure(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    calls = max(3, int(WINDOW * 1e6 / max(timed(fn, 3), 1.0)))
    t = [timed(fn, calls) for _ in range(ROUNDS)]
    return {"min": round(min(t), 2), "median": round(statistics.median(t), 2), "max": round(max(t), 2), "calls": calls}


def times():
    import lamb_cases as lac
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    out = {}
    dfm = mod("deform")
    M, H = 100000, 512
    x, bias, gp, gr, cs = rn(M, H), rn(H), rn(M, H), rn(M, H), torch.zeros(H, device=dev)
    act, _ = dfm._relu_bias(x, bias)
    out["mlp_relu_bias 100000x512"] = measure(lambda: dfm._relu_bias(x, bias))
    out["mlp_relu_backward 100000x512"] = measure(lambda: dfm._relu_backward(gp, act, gr, cs))
    L = _lib.lib()
    s = mod("_ops").stream(dev)
    N = 100000
    delta, xyz, rot, gx, grot = rn(N, 7), rn(N, 3), rn(N, 4), rn(N, 3), rn(N, 4)
    nx, nr, gd = torch.empty(N, 3, device=dev), torch.empty(N, 4, device=dev), torch.empty(N, 7, device=dev)
    out["deform_apply_forward 100000"] = measure(lambda: L.mgs_deform_apply_forward(N, xyz.data_ptr(), rot.data_ptr(), delta.data_ptr(),
                                                                                   nx.data_ptr(), nr.data_ptr(), s))
    out["deform_apply_backward 100000"] = measure(lambda: L.mgs_deform_apply_backward(N, rot.data_ptr(), delta.data_ptr(), gx.data_ptr(),
                                                                                     grot.data_ptr(), gd.data_ptr(), s))
    raw = rn(N, 26).requires_grad_(True)
    xin = rn(N, 3)
    epi = mod("regressor").gaussian_epilogue

    def epilogue():
        o = epi(raw, xin)
        torch.autograd.backward([o["scale"], o["rot"], o["opacity"]], [torch.ones_like(o["scale"]), torch.ones_like(o["rot"]),
                                                                      torch.ones_like(o["opacity"])])
        raw.grad = None
    out["gaussian_epilogue fwd+bwd 100000"] = measure(epilogue)
    inp = lac.make_inputs(dict(kind="mani", hidden=512, groups=[dict(lac.MANI)], K=1, seed=1))
    ps = [t.to(dev).requires_grad_(True) for t in inp["params"]]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(dev) * 0.02
    opt = mod("optim").FusedLamb(ps, **lac.MANI)
    out["fused_lamb step 62 tensors 5.7M"] = measure(opt.step)
    for name, shape in (("ss_final 64x100^3", (1, 64, 100, 100, 100)), ("ss1_latents 128x20^3", (1, 128, 20, 20, 20))):
        xs = (torch.randn(*shape, generator=g) * 0.3 + 0.5).to(dev).requires_grad_(True)
        gk, gm = rn(shape[0], 3 * shape[1]), rn(shape[0], shape[1])
        ss = mod("spatial_softmax").spatial_softmax3d
        with torch.no_grad():
            out[f"spatial_softmax forward {name}"] = measure(lambda: ss(xs, 0.01, with_max=True))

        def both():
            kp, mx = ss(xs, 0.01, with_max=True)
            torch.autograd.backward([kp, mx], [gk, gm])
            xs.grad = None
        out[f"spatial_softmax fwd+bwd {name}"] = measure(both)
        del xs
    xd, wd, bd = rn(1, 256, 52, 52, 52).requires_grad_(True), (rn(128, 256, 3, 3, 3) * 0.01).requires_grad_(True), rn(128).requires_grad_(True)
    gy = rn(1, 128, 50, 50, 50)
    dense = mod("dense").dense_conv3d

    def dense_step():
        y = dense(xd, wd, bd, 0.02)
        y.backward(gy)
        xd.grad = wd.grad = bd.grad = None
    out["dense_conv3d fwd+bwd final_50 (256->128, 3^3, 50^3)"] = measure(dense_step)
    del xd, wd, bd, gy
    src = rn(1, 128, 20, 20, 20).requires_grad_(True)
    up = rn(1, 128, 104, 104, 104)
    rp = mod("volume").resample_pad
    with torch.no_grad():
        out["resample_pad forward 128x20^3 x5 pad 2"] = measure(lambda: rp([src], 5, 2))

    def volume_step():
        rp([src], 5, 2).backward(up)
        src.grad = None
    out["resample_pad fwd+bwd 128x20^3 x5 pad 2"] = measure(volume_step)
    del src, up
    import loss_cases as lc
    for case in ("mani_step", "l2_norm_last"):
        c = lc.CASES[case]
        inp, _ = lc.make_inputs(case)
        col, fea = inp["color"].to(dev).requires_grad_(True), inp["feature"].to(dev).requires_grad_(True)
        t_rgb, t_emb = lc.lay_out(inp["gt_rgb"], c["layout"][0]).to(dev), lc.lay_out(inp["gt_embed"], c["layout"][1]).to(dev)
        rl = mod("losses").rendering_loss

        def loss_step():
            rl(col, t_rgb, fea, t_emb, weights=c["weights"], embed_loss_fn=c["fn"])[0].backward()
            col.grad = fea.grad = None
        out[f"rendering_loss fwd+bwd {case}"] = measure(loss_step)
    narrow = mod("narrow").narrow_conv3d
    for name, ext in (("100^3", (100, 100, 100)), ("50x50x51", (50, 50, 51))):   # (W no multiple of 4: the straddling threads)
        xn, wn, bn = rn(1, 128, *ext).requires_grad_(True), (rn(1, 128, 3, 3, 3) * 0.02).requires_grad_(True), rn(1).requires_grad_(True)
        gn = rn(1, 1, *ext)

        def narrow_step():
            narrow(xn, wn, bn, "replicate").backward(gn)
            xn.grad = wn.grad = bn.grad = None
        out[f"narrow_conv3d fwd+bwd trans_decoder 128->1 {name}"] = measure(narrow_step)
        del xn, wn, bn, gn
    return out


row = {"label": args.label, "build_id": _lib.build_id(), "lib": os.path.relpath(_lib.LIB_PATH, ROOT), "hashes": hashes()}
if not args.no_times:
    row["times_us"] = times()
print(json.dumps(row))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(row, f, indent=1)
    f.write("\n")

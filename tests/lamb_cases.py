"""Cases, inputs, the float64 reference, a plain-torch restatement and the comparison of tests/test_optim.py -- TEST
INFRASTRUCTURE, shared with tests/golden/make_golden_lamb.py (which records what `reference_run()` returns) so that the live
reference and the committed fixtures are checked by the same code.

The reference is ManiGaussian's optimizer itself, helpers/optim/lamb.py, executed unmodified on the CPU in float64 from
float32-representable seeded inputs, K steps with a fresh seeded gradient per step.  It exists only where a development copy
of the reference does (tests/ref_import.py's first candidate, $MGS_REFERENCE_ROOT); everywhere else the committed fixtures under tests/golden/optim/ stand in, and
`restate()` -- the rules of the algorithm written once more, vectorised over flat buffers -- is checked against every fixture to
1e-12 so that it can serve as the float64 truth at sizes the fixtures cannot hold.
"""
import importlib.util
import os

import numpy as np
import torch

import ref_import

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "optim")
EPS_REL = 1e-5          # the bound on m, v, the norms, the trust ratio, and epsilon of the parameter bound (see test_optim.py)
WHOLE = 64              # fixtures keep tensors up to this many elements whole, a stride of about this many of larger ones

MANI = dict(lr=5e-4, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-6)  # ManiGaussian_BC.yaml:42,46 + the Lamb defaults
# name: what builds the tensors ("mani": the 62 tensors of the NeuralRenderer at `hidden`; else a list of shapes), the groups
# (hyper-parameters + tensor indices; None: one group of everything), K steps, seed, gradient scale, and the case's twist
CASES = {
    "mani_small":        dict(kind="mani", hidden=64, groups=[dict(MANI)], K=3, seed=1),
    "mani_small_k20":    dict(kind="mani", hidden=64, groups=[dict(MANI)], K=20, seed=2),
    "wd0":               dict(shapes=[(40, 30), (30,), (30, 30)], groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0)],
                              K=4, seed=3, zero_grad_first_step=[0]),
    "zero_grad_with_wd": dict(shapes=[(40, 30), (30,), (30, 30)], groups=[dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)],
                              K=4, seed=4, zero_grad_always=[0]),
    "adam_flag":         dict(shapes=[(40, 30), (30,), (30, 30)], groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4)],
                              K=4, seed=5, adam=True),
    "clamp10":           dict(shapes=[(50, 40), (50, 40), (17,)], groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4)],
                              K=4, seed=6, norms={0: 31.0, 1: 9.99}),
    "grad_none":         dict(shapes=[(40, 30), (25, 7), (30,)], groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4)],
                              K=4, seed=7, grad_none=[1]),
    "two_groups":        dict(shapes=[(40, 30), (30,), (30, 30), (12, 5)],
                              groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0, idx=[0, 1]),
                                      dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.02, idx=[2, 3])], K=5, seed=8),
    "odd_sizes":         dict(shapes=[(1,), (3,), (5,), (4097,), (262145,), (13, 79)],
                              groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-4)], K=3, seed=9, offset_view=[5]),
    "eps_dominated":     dict(shapes=[(64, 33), (500,), (500,)], groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0)],
                              K=4, seed=10, grad_mag={0: "mixed", 1: 1e-12, 2: 1e3}),
}


# ---- the 62 tensors of the NeuralRenderer ------------------------------------------------------------------------------------
def mani_modules(hidden):
    """The trainable part of the NeuralRenderer: the encoder ResnetFC(39 -> 26), the 26 x 26 regressor and
    the deformation field's ResnetFC(73 -> 7); d_latent 128, 5 blocks, 3 lin_z.  This repository's own modules, on the CPU."""
    from manigaussian_amd import deform
    enc = deform.ResnetFC(39, d_out=26, n_blocks=5, d_latent=128, d_hidden=hidden, combine_layer=3)
    reg = torch.nn.Linear(26, 26)
    dfm = deform.ResnetFC(73, d_out=7, n_blocks=5, d_latent=128, d_hidden=hidden, combine_layer=3)
    return enc, reg, dfm


def mani_tensors(hidden, gen):
    """[(name, float32 tensor)] re-initialised from `gen` with the reference's rule (resnetfc.py:36-39,90,94,118): Kaiming-normal
    weights (std = sqrt(2 / fan_in)), zero biases, zero fc_1.weight -- independent of torch's global RNG."""
    out = []
    for prefix, mod in zip(("encoder", "regressor", "deform"), mani_modules(hidden)):
        for name, p in mod.named_parameters():
            if name.endswith("bias") or name.endswith("fc_1.weight"):
                t = torch.zeros(p.shape, dtype=torch.float32)
            else:
                t = torch.randn(p.shape, generator=gen, dtype=torch.float32) * float(np.sqrt(2.0 / p.shape[1]))
            out.append((f"{prefix}.{name}", t))
    return out


def make_inputs(case):
    """-> dict(names, params [float32 CPU tensors], groups [dict(lr, betas, eps, weight_decay, idx)], adam, K, seed, case)."""
    c = CASES[case] if isinstance(case, str) else case
    gen = torch.Generator().manual_seed(c["seed"])
    if c.get("kind") == "mani":
        named = mani_tensors(c["hidden"], gen)
    else:
        named = [(f"t{i}", torch.randn(s, generator=gen, dtype=torch.float32) * 0.1) for i, s in enumerate(c["shapes"])]
        for i, want in c.get("norms", {}).items():
            t = named[i][1]
            named[i] = (named[i][0], (t * (want / t.double().norm().item())).float())
    params = [t for _, t in named]
    groups = []
    for g in c["groups"]:
        g = dict(g)
        g.setdefault("idx", list(range(len(params))))
        groups.append(g)
    return dict(names=[n for n, _ in named], params=params, groups=groups, adam=bool(c.get("adam", False)), K=c["K"],
                seed=c["seed"], case=c)


def gradients(inp, k):
    """The gradients of step k (0-based): float32 CPU tensors, None for a parameter without one."""
    c = inp["case"]
    gen = torch.Generator().manual_seed(1000 * inp["seed"] + k + 17)
    out = []
    for i, p in enumerate(inp["params"]):
        g = torch.randn(p.shape, generator=gen, dtype=torch.float32) * 0.02
        mag = c.get("grad_mag", {}).get(i)
        if mag == "mixed":  # gradients of magnitude 1e-12 (sqrt(v) << eps) next to gradients of magnitude 1e+3
            unit = g / 0.02
            small = (torch.arange(p.numel()).view(p.shape) % 2 == 0)
            g = torch.where(small, unit * 1e-12, unit * 1e3)
        elif mag is not None:
            g = g / 0.02 * mag
        if i in c.get("zero_grad_always", []) or (k == 0 and i in c.get("zero_grad_first_step", [])):
            g = torch.zeros_like(g)
        out.append(None if i in c.get("grad_none", []) else g)
    return out


def assert_input_classes(case, inp, run):
    """The class every case is meant to hit, asserted on a float64 run of it (`run`: reference_run() or restate())."""
    c = CASES[case]
    st = run["stats"]  # [K, n, 3]
    names = inp["names"]
    if c.get("kind") == "mani":
        assert len(inp["params"]) == 62
        zero = [i for i, n in enumerate(names) if n.endswith("bias") or n.endswith("fc_1.weight")]
        live = [i for i in range(62) if i not in zero]
        assert len(zero) == 41 and all(inp["params"][i].abs().max() == 0 for i in zero)
        assert (st[0, zero, 0] == 0).all() and (st[0, zero, 2] == 1).all()          # weight_norm == 0 -> ratio 1 on step 1
        assert (st[0, live, 0] > 0).all() and (st[0, live, 2] != 1).all()           # ... and the computed ratio elsewhere
        assert (st[1, zero, 0] > 0).all() and (st[1, zero, 2] != 1).all()           # step 2: they have moved
    if case == "wd0":
        assert st[0, 0, 1] == 0 and st[0, 0, 0] > 0 and st[0, 0, 2] == 1 and st[1, 0, 1] > 0  # adam_norm == 0 -> ratio 1
    if case == "zero_grad_with_wd":
        assert (st[:, 0, 1] > 0).all() and run["path"][0] > 0 and (run["m"][0] == 0).all()   # moves by wd * p alone
    if case == "adam_flag":
        assert inp["adam"] and (st[:, :, 2] != 1).all()
    if case == "clamp10":
        assert (st[:, 0, 0] == 10).all() and (st[:, 1, 0] < 10).all() and (st[:, 1, 0] > 9.9).all()
        assert inp["params"][0].double().norm() > 30
    if case == "grad_none":
        assert torch.isnan(st[:, 1, :]).all() and run["path"][1] == 0 and not torch.isnan(st[:, [0, 2], :]).any()
    if case == "two_groups":
        assert len(inp["groups"]) == 2 and inp["groups"][0]["betas"] != inp["groups"][1]["betas"]
    if case == "odd_sizes":
        assert [p.numel() for p in inp["params"]][:5] == [1, 3, 5, 4097, 262145] and c["offset_view"] == [5]
    if case == "eps_dominated":
        g = gradients(inp, 0)
        assert 1e-13 < g[1].abs().median() < 1e-11 and 1e2 < g[2].abs().median() < 1e4
        a = g[0].abs().reshape(-1)
        assert a[0::2].max() < 1e-10 and a[1::2].median() > 1e2
        v1 = run["v"][1].abs().max().sqrt().item()
        assert v1 < 1e-3 * inp["groups"][0]["eps"]                                          # sqrt(v) << eps


# ---- the reference, executed in place --------------------------------------------------------------------------------------
def _lamb_path():
    for r in ref_import._CANDIDATES:
        f = os.path.join(r, "helpers", "optim", "lamb.py")
        if os.path.isfile(f):
            return f
    return None


def have_reference():
    return not os.environ.get("MGS_LAMB_FIXTURES_ONLY") and _lamb_path() is not None


_REF = []


def reference_class():
    if not _REF:
        spec = importlib.util.spec_from_file_location("_mgs_reference_lamb", _lamb_path())
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _REF.append(mod.Lamb)
    return _REF[0]


def _as_float(x):
    return float(x) if not isinstance(x, torch.Tensor) else float(x.item())


def reference_run(inp, dtype=torch.float64):
    """The reference `Lamb`, unmodified, K steps on the CPU in `dtype`.  -> dict(stats [K,n,3] float64 (weight_norm, adam_norm,
    recorded trust_ratio; NaN for a parameter without state), path [n] = sum_k max |delta p_k|, p, m, v: lists of final
    tensors (m, v zeros for a parameter without state), steps [n])."""
    Lamb = reference_class()
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in inp["params"]]
    groups = [dict(params=[ps[i] for i in g["idx"]], lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
              for g in inp["groups"]]
    opt = Lamb(groups, adam=inp["adam"])
    n, K = len(ps), inp["K"]
    stats = torch.full((K, n, 3), float("nan"), dtype=torch.float64)
    path = torch.zeros(n, dtype=torch.float64)
    for k in range(K):
        before = [p.detach().clone() for p in ps]
        for p, g in zip(ps, gradients(inp, k)):
            p.grad = None if g is None else g.to(dtype)
        opt.step()
        for i, p in enumerate(ps):
            path[i] += (p.detach() - before[i]).abs().max().double()
            st = opt.state.get(p)
            if st:
                stats[k, i] = torch.tensor([_as_float(st["weight_norm"]), _as_float(st["adam_norm"]), _as_float(st["trust_ratio"])],
                                           dtype=torch.float64)
    z = [opt.state.get(p) or {} for p in ps]
    return dict(stats=stats, path=path, p=[p.detach().clone() for p in ps],
                m=[s["exp_avg"].clone() if s else torch.zeros_like(p.detach()) for s, p in zip(z, ps)],
                v=[s["exp_avg_sq"].clone() if s else torch.zeros_like(p.detach()) for s, p in zip(z, ps)],
                steps=[int(s.get("step", 0)) for s in z])


# ---- the rules once more, vectorised over flat buffers ---------------------------------------------------------------------
def restate(inp, dtype=torch.float64, params=None, grads_of_step=None, K=None):
    """LAMB as ManiGaussian runs it, for ALL tensors at once: every tensor is a segment of one flat buffer, per-tensor sums are
    index_add_ over a segment id, per-tensor scalars are gathered back by it.  Same result dict as reference_run()."""
    params = inp["params"] if params is None else params
    grads_of_step = grads_of_step or (lambda k: gradients(inp, k))
    K = inp["K"] if K is None else K
    n = len(params)
    numel = torch.tensor([p.numel() for p in params])
    seg = torch.repeat_interleave(torch.arange(n), numel)
    P = torch.cat([p.reshape(-1).to(dtype) for p in params])
    M, V = torch.zeros_like(P), torch.zeros_like(P)
    hyp = torch.zeros(n, 7, dtype=dtype)  # lr, beta1, 1 - beta1, beta2, 1 - beta2, eps, weight_decay
    for g in inp["groups"]:
        b1, b2 = g["betas"]
        hyp[g["idx"]] = torch.tensor([g["lr"], b1, 1 - b1, b2, 1 - b2, g["eps"], g["weight_decay"]], dtype=dtype)
    lr, b1, omb1, b2, omb2, eps, wd = (hyp[:, j] for j in range(7))
    stats = torch.full((K, n, 3), float("nan"), dtype=torch.float64)
    path = torch.zeros(n, dtype=torch.float64)
    steps = torch.zeros(n, dtype=torch.long)

    def per_tensor_sum(x):
        return torch.zeros(n, dtype=dtype).index_add_(0, seg, x)

    for k in range(K):
        gs = grads_of_step(k)
        has = torch.tensor([g is not None for g in gs])                                      # rule 7: no gradient, no step
        G = torch.cat([(torch.zeros(p.numel()) if g is None else g.reshape(-1)).to(dtype) for g, p in zip(gs, params)])
        act = has[seg]
        M = torch.where(act, M * b1[seg] + G * omb1[seg], M)                                 # rule 1, no bias correction
        V = torch.where(act, V * b2[seg] + G * G * omb2[seg], V)
        wn = per_tensor_sum(P * P).sqrt().clamp(0, 10)                                    # rule 2
        U = M / (V.sqrt() + eps[seg])                                                        # rule 3
        U = torch.where((wd != 0)[seg], U + wd[seg] * P, U)
        an = per_tensor_sum(torch.where(act, U * U, torch.zeros_like(U))).sqrt()          # rule 4
        tr = torch.where((wn == 0) | (an == 0), torch.ones_like(wn), wn / an)
        applied = torch.ones_like(tr) if inp["adam"] else tr                                 # rule 5
        D = torch.where(act, -(lr * applied)[seg] * U, torch.zeros_like(U))                  # rule 6
        newP = P + D
        path += torch.stack([x.max() for x in torch.split((newP - P).abs(), numel.tolist())]).double()
        P = newP
        stats[k, has] = torch.stack([wn, an, tr], 1).double()[has]
        steps += has.long()
    cut = lambda X: [x.view(p.shape) for x, p in zip(torch.split(X, numel.tolist()), params)]  # noqa: E731
    return dict(stats=stats, path=path, p=cut(P), m=cut(M), v=cut(V), steps=steps.tolist())


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def sample_index(numel):
    """Fixed element sample of a tensor: all of a small one; of a large one a stride, the first and last elements and the
    elements around every chunk boundary of the kernels (4096)."""
    if numel <= WHOLE:
        return torch.arange(numel)
    idx = set(range(0, numel, max(1, numel // WHOLE)))
    idx.update((0, 1, numel - 2, numel - 1))
    for b in range(4096, numel, 4096 * max(1, numel // 4096 // 4)):
        idx.update((b - 1, b))
    return torch.tensor(sorted(idx), dtype=torch.long)


def fixture_path(case):
    return os.path.join(GOLDEN_DIR, case + ".npz")


def to_fixture(run):
    """What a fixture keeps of a float64 run: the statistics of every step, the paths, per-tensor maxima of |p|, |m|, |v| (the
    scales of the bounds) and p, m, v after the last step at sample_index()."""
    d = dict(stats=run["stats"].numpy(), path=run["path"].numpy(), steps=np.asarray(run["steps"], dtype=np.int32))
    for key in ("p", "m", "v"):
        d[key + "max"] = np.asarray([t.abs().max().item() for t in run[key]], dtype=np.float64)
        d[key] = np.concatenate([t.reshape(-1)[sample_index(t.numel())].double().numpy() for t in run[key]])
    return d


def load_fixture(case):
    z = np.load(fixture_path(case))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def fixture_of_run(run):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in to_fixture(run).items()}


def expected(case, inp):
    """What to compare against, in fixture form: the live float64 reference where the development copy exists, else the
    committed fixture (recorded from the same computation)."""
    if have_reference():
        return dict(fixture_of_run(reference_run(inp)), source="reference")
    return dict(load_fixture(case), source="fixture")


def compare(name, got, exp, K, report=print, eps=EPS_REL):
    """got: a result dict in the form of reference_run() from the code under test (CPU tensors), exp: fixture form.  Prints
    every figure, then asserts the bounds of tests/test_optim.py's docstring."""
    failures = []
    gs, es = got["stats"].double(), exp["stats"].double()
    n = es.shape[1]
    off = 0
    worst = dict(stat=0.0, m=0.0, v=0.0, p=0.0)
    for i in range(n):
        numel = got["p"][i].numel()
        idx = sample_index(numel)
        sl = slice(off, off + idx.numel())
        off += idx.numel()
        skipped = int(exp["steps"][i]) == 0
        if int(got["steps"][i]) != int(exp["steps"][i]):
            failures.append((i, "steps", int(got["steps"][i]), int(exp["steps"][i])))
        for k in range(es.shape[0]):
            e, g = es[k, i], gs[k, i]
            if torch.isnan(e).all():
                if not torch.isnan(g).all():
                    failures.append((i, k, "statistics of a skipped step", g.tolist()))
                continue
            # discrete: which branch the ratio took
            if (e[0] == 0) != (g[0] == 0) or (e[1] == 0) != (g[1] == 0):
                failures.append((i, k, "zero test", g.tolist(), e.tolist()))
                continue
            if (e[0] == 0 or e[1] == 0) and g[2] != 1:
                failures.append((i, k, "degenerate ratio is not 1", g.tolist()))
            for j, what in enumerate(("weight_norm", "adam_norm", "trust_ratio")):
                err = abs(g[j] - e[j]).item() / abs(e[j]).item() if e[j] != 0 else abs(g[j]).item()
                worst["stat"] = max(worst["stat"], err)
                if not err <= eps:
                    failures.append((i, k, what, g[j].item(), e[j].item(), err))
        for key in ("m", "v"):
            g = got[key][i].reshape(-1)[idx].double()
            err, scale = (g - exp[key][sl]).abs().max().item(), exp[key + "max"][i].item()
            worst[key] = max(worst[key], err / scale if scale else err)
            if not err <= eps * scale:
                failures.append((i, key, err, scale))
        g = got["p"][i].reshape(-1)[idx].double()
        err = (g - exp["p"][sl]).abs().max().item()
        if skipped:
            if err != 0:
                failures.append((i, "a skipped parameter changed", err))
            continue
        bound = K * 2.0 ** -23 * exp["pmax"][i].item() + eps * exp["path"][i].item()
        worst["p"] = max(worst["p"], err / bound if bound else err)
        if not err <= bound:
            failures.append((i, "p", err, bound))
    assert off == exp["p"].numel(), (off, exp["p"].numel())
    report(f"  {name}: worst statistic rel {worst['stat']:.3g}, m {worst['m']:.3g}, v {worst['v']:.3g} (of the tensor's max; bound "
           f"{eps:g}), parameters at {worst['p']:.3g} of their bound")
    assert not failures, (name, exp.get("source"), failures[:8])
    return worst

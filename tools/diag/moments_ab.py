"""A/B of the staged-tile moment families (csrc/gmm.hip, probe.hip, strata.hip) between two builds of the library (FRL_BUILD_TAG builds; the
empty tag is the default library).

  python tools/diag/moments_ab.py bits --tags parent,   every output tensor of gmm_pivot / em_step / m_step (EM, Lloyd, init) / score,
                                                        probe_pivot / accumulate / evaluate (with and without pred) and strata_moments
                                                        (both modes) at the shapes of the GPU tests, workgroups 0, 1 and 3, hashed in one
                                                        child process per library and compared
  python tools/diag/moments_ab.py time --tags parent,   per route the median of 200 calls (HIP events around the call) at the shape of its
                                                        bench tool, three rounds, the libraries alternating, one child process per library
                                                        and round
Both print one line `JSON {...}`.
"""
import hashlib, json, os, subprocess, sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
ROUNDS, LAUNCHES = 3, 200
DEV = "cuda:0"


def _setup():
    for p in ("vq-vae_amd", "oracle", "tests"):
        sys.path.insert(0, os.path.join(ROOT, p))
    import torch
    from frl_hip import ops
    return torch, ops


def bits():
    torch, ops = _setup()
    import numpy as np
    import gmm_cases as G
    import strata_cases as SC
    import test_gpu_probe as TP
    import test_gpu_strata as TS
    from frl_hip import probe as P
    out = {}

    def put(key, **tensors):
        for name, t in tensors.items():
            if t is not None:
                out[f"{key} {name}"] = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]

    def dev(a):
        return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)

    for case in G.STEP_CASES:
        inp = G.make_inputs(case)
        X, w = dev(inp["X"]), dev(inp["w"])
        n, d = X.shape
        k = len(inp["weights_init"])
        for wg in (0, 1, 3):
            ws = ops.gmm_workspace(n, d, k, DEV, wg)
            pivot = ops.gmm_pivot(X, ws)
            for mode, hard in (("em", False), ("lloyd", True), ("init", True)):
                pi, mu, var = dev(inp["weights_init"]), dev(inp["means_init"]), dev(inp["variances_init"])
                mc = (mu.double() - pivot.double()).float()
                state = torch.zeros(2, dtype=torch.int32, device=DEV)
                hist = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
                ops.gmm_em_step(X, w, pivot, pi, mc, var, state, ws, hard=hard, workgroups=wg)
                ops.gmm_m_step(n, pivot, pi, mu, mc, var, state, ws, hist if mode == "em" else None, G.REG_COVAR, G.TOL,
                               {"em": ops.GMM_M_EM, "lloyd": ops.GMM_M_LLOYD, "init": ops.GMM_M_INIT}[mode], wg)
                put(f"gmm {case} wg={wg} {mode}", pivot=pivot, weights=pi, means=mu, means_c=mc, variances=var, state=state, history=hist)
            if wg == 0:
                lse, labels, resp = ops.gmm_score(X, pivot, pi, mc, var, want_resp=True)
                put(f"gmm {case} score", lse=lse, labels=labels, resp=resp)

    for case in "abcdefg":
        r = TP._inputs(case)
        a, bs, hw = P._sources(r["feats"], True)
        y, _ = P._rows(r["targets"], True, "targets")
        m = P._mask_rows(r["mask"], hw, r["halo"])
        d, cy = a.shape[3] + (0 if bs is None else bs.shape[3]), y.shape[3]
        g = torch.Generator().manual_seed(d + cy)
        wc, bc = (torch.randn(d, cy, generator=g) / d ** 0.5).to(DEV), torch.randn(cy, generator=g).to(DEV)
        for wg in (0, 1, 3):
            ws = ops.probe_workspace(d, cy, DEV, wg)
            pivot = ops.probe_pivot(a, bs, y, m, ws)
            S = torch.zeros(d + cy + 1, d + cy + 1, dtype=torch.float64, device=DEV)
            n = torch.zeros(1, dtype=torch.int64, device=DEV)
            for _ in range(2):                                                   # the second call adds to the state of the first
                ops.probe_accumulate(a, bs, y, m, pivot, S, n, ws, wg)
            put(f"probe {case} wg={wg}", pivot=pivot, S=S, n=n)
            for want_pred in (False, True):
                E = torch.zeros(cy, 3, dtype=torch.float64, device=DEV)
                ne = torch.zeros(1, dtype=torch.int64, device=DEV)
                pred = ops.probe_evaluate(a, bs, y, m, pivot, wc, bc, E, ne, ws, want_pred, wg)
                put(f"probe {case} wg={wg} evaluate pred={want_pred}", E=E, n=ne, pred=pred)

    cases = [(SC.moment_case(shape, g), f"{shape} G={g}") for shape in SC.MOMENT_SHAPES for g in SC.MOMENT_GROUPS]
    cases += [(SC.moment_case(shape, g, seed=3), f"{shape} G={g} seed=3") for shape, g in (((2, 5, 300, 12), 20), ((1, 3, 70, 128), 127), ((1, 2, 70, 6), 20))]
    cases += [(SC.moment_case((1, 2, 66000, 4), 200, seed=5), "many tiles")]
    for temporal in (False, True):
        cases.append((SC.moment_case((2, 5, 300, 12), 20, as_float=True, per_step_mask=not temporal, seed=1), f"float codes temporal={temporal}"))
        for c, what in cases:
            if c["mask"].shape[1] > 1 and temporal:
                continue
            for wg in (0, 1, 3):
                for pivot in (None, np.full(c["X"].shape[-1], 0.25, np.float32)):
                    gm = TS._fit_moments(c, temporal, pivot=pivot, workgroups=wg)
                    put(f"strata {what} temporal={temporal} wg={wg} pivot={'mean' if pivot is None else 'given'}", count=gm._count, S1=gm._s1,
                        S2=gm._s2, SW=gm._sw, unmatched=gm._unm, pivot=gm._pivot)
    return out


def time_routes():
    torch, ops = _setup()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gmm_bench, probe_bench, strata_bench
    from frl_hip import probe as P
    from frl_hip.strata import GroupedMoments
    routes = {}
    for n, d, k in gmm_bench.SHAPES:
        Xc, pi0, mu0, var0 = gmm_bench.make(n, d, k, 1000 + k)
        X, p0, m0, v0 = Xc.to(DEV), pi0.to(DEV), mu0.to(DEV), var0.to(DEV)
        ws = ops.gmm_workspace(n, d, k, DEV)
        pivot = ops.gmm_pivot(X, ws)
        pi, mu, var, mc = p0.clone(), m0.clone(), v0.clone(), (m0.double() - pivot.double()).float()
        hist, state = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)

        def gmm(X=X, pivot=pivot, pi=pi, mu=mu, var=var, mc=mc, state=state, hist=hist, ws=ws, n=n):
            state.zero_()
            ops.gmm_em_step(X, None, pivot, pi, mc, var, state, ws)
            ops.gmm_m_step(n, pivot, pi, mu, mc, var, state, ws, hist, gmm_bench.REG, gmm_bench.TOL, ops.GMM_M_EM)
        routes[f"gmm em_step + m_step N{n} D{d} K{k}"] = gmm
    z, y, m = probe_bench.make_static(16, 256, 256, 64, 5, 1.0, 7)
    a, bs, hw = P._sources(z, False)
    yr, _ = P._rows(y, False, "targets")
    mr = P._mask_rows(m, hw, 0)
    pws = ops.probe_workspace(64, 5, DEV)
    ppivot = ops.probe_pivot(a, bs, yr, mr, pws)
    S, cnt = torch.zeros(70, 70, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    routes["probe accumulate 16x256x256 D64 Cy5"] = lambda: ops.probe_accumulate(a, bs, yr, mr, ppivot, S, cnt, pws)
    zt2, zp2, y2, m2 = probe_bench.make_phase(16, 8, 256, 256, 64, 12, 7, 11)
    a2, b2, hw2 = P._sources((zt2, zp2), False)
    y2r, _ = P._rows(y2, False, "targets")
    m2r = P._mask_rows(m2, hw2, 16)
    pws2 = ops.probe_workspace(76, 7, DEV)
    ppivot2 = ops.probe_pivot(a2, b2, y2r, m2r, pws2)
    S2, cnt2 = torch.zeros(84, 84, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    routes["probe accumulate 16x8x256x256 D64+12 Cy7 halo16"] = lambda: ops.probe_accumulate(a2, b2, y2r, m2r, ppivot2, S2, cnt2, pws2)
    for g in (20, 200):                                                          # 200 codes: two windows of the vocabulary per call
        vocab, codes, _, mask, gamma, zt = strata_bench.make(g, 1.0, True, 5)
        spivot = gamma[mask].mean(dim=0).cpu().numpy()
        mom = GroupedMoments(vocab.cpu().tolist(), strata_bench.D, pivot=spivot)
        tmp = GroupedMoments(vocab.cpu().tolist(), strata_bench.D, temporal=True, pivot=spivot)
        routes[f"strata moments 16x256x256 D12 G{g}"] = lambda mom=mom, gamma=gamma, codes=codes, mask=mask: mom.partial_fit(gamma, codes, mask)
        routes[f"strata temporal moments 16x15x256x256 D12 G{g}"] = lambda tmp=tmp, zt=zt, codes=codes, mask=mask: tmp.partial_fit(zt, codes, mask)
    res = {}
    for name, fn in routes.items():
        for _ in range(5):
            fn()
        ts = []
        for _ in range(LAUNCHES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        res[name] = sorted(ts)[LAUNCHES // 2]
    return res


def child(mode, tag):
    env = dict(os.environ)
    env.pop("FRL_HIP_LIB_TAG", None)
    if tag:
        env["FRL_HIP_LIB_TAG"] = tag
    out = subprocess.run([sys.executable, os.path.abspath(__file__), mode, "--child"], env=env, capture_output=True, text=True, timeout=900)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    if out.returncode != 0 or not line:
        sys.stderr.write(out.stdout + out.stderr)
        sys.exit(f"library '{tag}' failed (exit code {out.returncode})")
    return json.loads(line[0][7:])


if __name__ == "__main__":
    mode = sys.argv[1]
    if "--child" in sys.argv:
        print("RESULT " + json.dumps(bits() if mode == "bits" else time_routes()))
        sys.exit(0)
    tags = sys.argv[sys.argv.index("--tags") + 1].split(",")
    if mode == "bits":
        a = child("bits", tags[0])
        print(f"'{tags[0]}' done: {len(a)} tensors", flush=True)
        b = child("bits", tags[1])
        diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
        print("JSON " + json.dumps({"tensors": len(a), "differing": diff, "verdict": "identical" if not diff and len(a) == len(b) else "DIFFERENT"}))
        sys.exit(1 if diff else 0)
    allres = {t or "default": {} for t in tags}
    for rnd in range(ROUNDS):
        for t in tags:
            for k, v in child("time", t).items():
                allres[t or "default"].setdefault(k, []).append(round(v, 2))
            print(f"round {rnd} '{t}' done", flush=True)
    print("JSON " + json.dumps(allres))

"""Diagonal-covariance GMM micro-benchmark, one JSON line per shape (appended to --out): the fused EM iteration of csrc/gmm.hip
(ops.gmm_em_step + ops.gmm_m_step, three launches) and a whole DiagGMM.fit against
  torch ops:  the same formulas composed from stock torch ops on the same device in the same run (sklearn's expansion of the
              log-probabilities as three matrix products, logsumexp, exp, the two moment products), which writes [N][K] arrays several
              times per iteration;
  sklearn:    sklearn.mixture.GaussianMixture(covariance_type="diag") on the CPU, where it imports (--sklearn-iters iterations from the
              same initial parameters, timed as a whole and divided; the whole fit only at the small shape).
Shapes: N = 500 000, D = 64, K in {5, 50} (the type sweep's ends) and N = 20 000, D = 36, K = 5 (a phase sweep).  Data: K blobs; initial
parameters: K data rows, the column variance, equal weights.
Per iteration: 5 warm-up iterations, then the median / min of 30, HIP events around each Python call and a device synchronise after it, the
sides alternating; every timed iteration starts from the same parameters.  A second pass records the library's per-kernel event times.
Achieved bytes/s of X = N D 4 / the E kernel's time, against an HBM peak of 8 TB/s.
Usage: python tools/gmm_bench.py [--out profiles/gmm_bench.jsonl] [--sklearn-iters 2]"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip import ops  # noqa: E402
from frl_hip.clustering import DiagGMM  # noqa: E402

DEV = "cuda:0"
SHAPES = ((500_000, 64, 5), (500_000, 64, 50), (20_000, 36, 5))
HBM_PEAK = 8.0e12
REG, TOL, MAX_ITER = 1e-6, 1e-3, 200


def make(n, d, k, seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(k, d, generator=g)
    scales = 0.5 + torch.rand(k, d, generator=g)
    comp = torch.randint(0, k, (n,), generator=g)
    X = (centres[comp] + torch.randn(n, d, generator=g) * scales[comp]).contiguous()
    rows = torch.randperm(n, generator=g)[:k]
    return X, torch.full((k,), 1.0 / k), X[rows].clone(), X.var(0, unbiased=False).repeat(k, 1)


def torch_em(X, X2, pi, mu, var):
    d = X.shape[1]
    prec = 1.0 / var
    lp = -0.5 * (d * math.log(2 * math.pi) + (mu * mu * prec).sum(1) - 2.0 * (X @ (mu * prec).T) + X2 @ prec.T) + 0.5 * prec.log().sum(1) + pi.log()
    lse = torch.logsumexp(lp, 1)
    r = torch.exp(lp - lse[:, None])
    nk = r.sum(0) + 10 * 2.220446049250313e-16
    m = (r.T @ X) / nk[:, None]
    v = (r.T @ X2) / nk[:, None] - m * m + REG
    return nk / nk.sum(), m, v, lse.mean()


def timed(fns, n=30, warm=5):
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(n):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return [(round(sorted(t)[len(t) // 2], 1), round(min(t), 1)) for t in ts]


def kernel_times(fn):
    ops.kernel_timing(True)
    ops.kernel_timing_report()
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    kernels = {k: round(v[1] / v[0] * 1e3, 1) for k, v in ops.kernel_timing_report().items()}
    ops.kernel_timing(False)
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sklearn-iters", type=int, default=2)
    args = ap.parse_args()
    lines = []
    for n, d, k in SHAPES:
        Xc, pi0, mu0, var0 = make(n, d, k, 1000 + k)
        X = Xc.to(DEV)
        X2 = X * X                                                                # the composition squares X once per fit, not per iteration
        p0, m0, v0 = pi0.to(DEV), mu0.to(DEV), var0.to(DEV)
        ws = ops.gmm_workspace(n, d, k, DEV)
        pivot = ops.gmm_pivot(X, ws)
        pi, mu, var, mc = p0.clone(), m0.clone(), v0.clone(), (m0.double() - pivot.double()).float()
        hist = torch.zeros(1, dtype=torch.float64, device=DEV)
        state = torch.zeros(2, dtype=torch.int32, device=DEV)

        def fused():
            pi.copy_(p0), var.copy_(v0), mc.copy_(m0 - pivot), state.zero_()
            ops.gmm_em_step(X, None, pivot, pi, mc, var, state, ws)
            ops.gmm_m_step(n, pivot, pi, mu, mc, var, state, ws, hist, REG, TOL, ops.GMM_M_EM)

        def stock():
            return torch_em(X, X2, p0, m0, v0)

        (fm, fmin), (sm, smin) = timed([fused, stock])
        fused()
        want = stock()
        dev_mu = float((mu - want[1]).abs().max())
        kern = kernel_times(fused)
        e_us = next((v for kk, v in kern.items() if "gmm_e_kernel" in kk), None)

        def fit_fused():
            return DiagGMM(k, tol=TOL, reg_covar=REG, max_iter=MAX_ITER, weights_init=pi0, means_init=mu0, precisions_init=1.0 / var0.double()).fit(X)

        def fit_stock():
            a, prev = (p0, m0, v0), -math.inf
            for it in range(MAX_ITER):
                *a, lb = torch_em(X, X2, *a)
                lb = float(lb)                                                    # the host read sklearn's loop makes every iteration
                if abs(lb - prev) < TOL:
                    break
                prev = lb
            return it + 1

        fit_fused(), fit_stock()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = fit_fused()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        it_stock = fit_stock()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        line = {"case": "gmm_diag", "N": n, "D": d, "K": k, "fused_iter_us_median": fm, "fused_iter_us_min": fmin,
                "torch_ops_iter_us_median": sm, "torch_ops_iter_us_min": smin, "speedup_at_median": round(sm / fm, 2),
                "fused_launches_per_iter": 3, "fused_kernel_us_mean_of_10": kern, "means_max_dev_vs_torch_ops": dev_mu,
                "x_bytes_per_s_e_kernel": None if not e_us else round(n * d * 4 / (e_us * 1e-6), -9), "hbm_peak_bytes_per_s": HBM_PEAK,
                "x_fraction_of_hbm_peak": None if not e_us else round(n * d * 4 / (e_us * 1e-6) / HBM_PEAK, 4),
                "fused_fit_ms": round((t1 - t0) * 1e3, 2), "fused_fit_n_iter": g.n_iter_, "fused_fit_launches": g.launches_,
                "torch_ops_fit_ms": round((t2 - t1) * 1e3, 2), "torch_ops_fit_n_iter": it_stock,
                "timing": "iteration: HIP events around the Python call, a synchronise after each, the sides alternating; fit: wall clock of "
                          "one call after one warm-up call"}
        try:
            import warnings
            from sklearn.mixture import GaussianMixture
            Xn = Xc.double().numpy()
            kw = dict(covariance_type="diag", tol=TOL, reg_covar=REG, weights_init=(pi0.double() / pi0.double().sum()).numpy(),
                      means_init=mu0.double().numpy(), precisions_init=(1.0 / var0.double()).numpy())
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                GaussianMixture(k, max_iter=args.sklearn_iters, **kw).fit(Xn)
                line["sklearn_cpu_iter_ms"] = round((time.perf_counter() - t0) * 1e3 / args.sklearn_iters, 1)
                line["sklearn_cpu_threads"] = torch.get_num_threads()
                if n <= 20_000:
                    t0 = time.perf_counter()
                    sk = GaussianMixture(k, max_iter=MAX_ITER, **kw).fit(Xn)
                    line["sklearn_cpu_fit_ms"], line["sklearn_cpu_fit_n_iter"] = round((time.perf_counter() - t0) * 1e3, 1), int(sk.n_iter_)
        except ImportError:
            line["sklearn_cpu_iter_ms"] = None
        lines.append(line)
        print(json.dumps(line), flush=True)
        del X, X2
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

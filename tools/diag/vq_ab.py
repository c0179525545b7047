"""A/B of the VQ assignment between two builds of the library (FRL_BUILD_TAG builds; the empty tag is the default library).

  python tools/diag/vq_ab.py bits --tags parent,     every tensor the four test_vq_assign_* / test_vq_golden_fixture tests look at (idx, z_q,
                                                     counts, the four stats words), at their parametrisations, hashed in one child process per
                                                     library and compared
  python tools/diag/vq_ab.py time --tags parent,     per route the median of 200 launches (HIP events around the C-ABI call, prepared image),
                                                     five rounds, the libraries alternating, one child process per library and round
Both print one line `JSON {...}`.
"""
import hashlib, json, os, subprocess, sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
ROUNDS, LAUNCHES = 5, 200
# (name, rows, K, d, dtype, stream hook); 262144 rows = BASELINE's batch of 256 tiles
ROUTES = [("stream bf16 K512 d64", 262144, 512, 64, "bf16", -1),
          ("resident bf16 K512 d64", 262144, 512, 64, "bf16", 0),
          ("chunked f32 K512 d64 (two chunks of 256 codes)", 262144, 512, 64, "f32", -1),
          ("resident f32 K256 d64", 262144, 256, 64, "f32", -1),
          ("chunked bf16 K1024 d64", 262144, 1024, 64, "bf16", -1),
          ("chunked bf16 K8192 d128", 262144, 8192, 128, "bf16", -1)]


def _setup():
    for p in ("vq-vae_amd", "oracle", "tests"):
        sys.path.insert(0, os.path.join(ROOT, p))
    import torch
    from frl_hip import ops
    return torch, ops


def _params(fn):
    """[(argnames, values)] of the parametrize marks of a test function, innermost first"""
    return [(m.args[0].split(","), m.args[1]) for m in fn.pytestmark if m.name == "parametrize"]


def bits():
    torch, ops = _setup()
    import numpy as np
    import test_gpu_kernels_basic as T
    dev, out = "cuda:0", {}

    def put(key, res):
        idx, zq, stats, counts = res
        for name, t in (("idx", idx), ("zq", zq), ("counts", counts), ("stats", stats)):
            out[f"{key} {name}"] = hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]

    def both(key, z, e):
        put(key, ops.vq_assign(z.to(dev), e.to(dev)))
        prep = ops.vq_prepare(e.to(dev), z.shape[0], z.dtype)
        for rep in range(2):
            put(f"{key} prepared#{rep}", ops.vq_assign(z.to(dev), e.to(dev), prep))

    (_, shapes), (_, dtypes) = _params(T.test_vq_assign_bit_exact)
    for dtype in dtypes:
        for N, K, d, ties in shapes:
            g = torch.Generator().manual_seed(N + K + d)
            z, e = torch.randn(N, d, generator=g), torch.randn(K, d, generator=g)
            if ties and K > 8 and N > 8:
                e[K - 1] = e[3]; z[5] = 0.0; e[7] = -e[2]; z[6] = e[4]
            both(f"bit_exact {dtype} {N} {K} {d} {ties}", z.to(dtype), e)
    (_, shapes), (_, dtypes) = _params(T.test_vq_assign_every_row_is_a_tie)
    for dtype in dtypes:
        for N, K, d, dup in shapes:
            g = torch.Generator().manual_seed(N + K + dup)
            e = torch.randn(K // dup, d, generator=g).repeat_interleave(dup, dim=0).contiguous()
            both(f"every_row_is_a_tie {dtype} {N} {K} {d} {dup}", torch.randn(N, d, generator=g).to(dtype), e)
    ((_, cases),) = _params(T.test_vq_assign_streaming_kernel_matches_resident)
    for N, K, case in cases:
        d = 64
        g = torch.Generator().manual_seed(N + K)
        z = torch.randn(N, d, generator=g)
        if case.startswith("dup"):
            e = torch.randn(K // int(case[3:]), d, generator=g).repeat_interleave(int(case[3:]), dim=0).contiguous()
        elif case == "live":
            e = z[torch.randperm(N, generator=g)[:K]].to(torch.bfloat16).float().contiguous()
        else:
            e = torch.randn(K, d, generator=g)
        if case == "ties":
            e[K - 1] = e[3]; z[5] = 0.0; e[7] = -e[2]; z[6] = e[4]
        if case == "nan":
            z[17] = float("nan"); z[300, 3] = float("inf"); z[4097] = float("-inf")
        for nt in (0, 1, 2, 4):
            prev = ops.vq_stream_tiles(nt)
            try:
                both(f"streaming {N} {K} {case} tiles={nt}", z.to(torch.bfloat16), e)
            finally:
                ops.vq_stream_tiles(prev)
    fx = np.load(os.path.join(ROOT, "tests", "golden", "vq_seed7.npz"))
    both("golden", torch.from_numpy(fx["z"]), torch.from_numpy(fx["e"]))
    return out


def time_routes():
    torch, ops = _setup()
    dev, res = "cuda:0", {}
    for name, N, K, d, dt, hook in ROUTES:
        dtype = torch.bfloat16 if dt == "bf16" else torch.float32
        g = torch.Generator().manual_seed(0)
        z = torch.randn(N, d, generator=g).to(dtype).to(dev)
        g.manual_seed(1)
        E = z[torch.randperm(N, generator=g)[:K].to(dev)].float().contiguous()          # a live codebook: rows drawn from z
        prev = ops.vq_stream_tiles(hook)
        prep = ops.vq_prepare(E, N, dtype)
        for _ in range(5):
            ops.vq_assign(z, E, prep)
        ts = []
        for _ in range(LAUNCHES):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.vq_assign(z, E, prep)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ops.vq_stream_tiles(prev)
        res[name] = sorted(ts)[LAUNCHES // 2]
        del z, E, prep
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
        a, b = child("bits", tags[0]), child("bits", tags[1])
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

"""dec_mse_bwd in isolation at the two shapes of the train step (12-channel latents, 1.31 M rows; 64-channel latents, 262 k rows), through
frl_decoder_mse_bwd (kernel + pack + slab reduce) and the one-pass frl_decoder_mse_fwd_bwd (kernel + finalize): two 4-wave subgroups per
workgroup vs the lockstep workgroup (64 channels: the 8-wave kernel at two waves per SIMD vs the 4-wave one; the switch is
frl_decoder_mse_bwd_subgroups).

  python tools/diag/dec_sg_ab.py                    this library, five rounds in one process, subgroups / lockstep interleaved
  python tools/diag/dec_sg_ab.py --tags parent,     libraries against each other (FRL_BUILD_TAG builds; the empty tag is the default
                                                    library): five rounds, the libraries interleaved, one child process per library and round
"""
import json, os, subprocess, sys
ROUNDS = 5
CASES = [("cz12 1.31M", 256 * 5 * 1024, 12), ("cz64 262k", 256 * 1024, 64)]


def measure(rounds):
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "vq-vae_amd"))
    import torch
    from frl_hip import ops, _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    res = {}
    for name, P, cz in CASES:
        z = torch.randn(P, cz, generator=g).bfloat16().cuda()
        tgt = torch.randn(P, 64, generator=g).bfloat16().cuda()
        w1 = (torch.randn(128, cz, generator=g) / cz ** 0.5).cuda(); b1 = torch.zeros(128).cuda()
        w2 = (torch.randn(64, 128, generator=g) / 128 ** 0.5).cuda(); b2 = torch.zeros(64).cuda()
        stats, _ = ops.decoder_mse_fwd(z, w1, b1, w2, b2, tgt, None)
        gs = torch.ones(1, device="cuda")
        calls = {"bwd": lambda: ops.decoder_mse_bwd(z, w1, b1, w2, b2, tgt, None, gs, stats),
                 "onepass": lambda: ops.decoder_mse_fwd_bwd(z, w1, b1, w2, b2, tgt, None, gs)}
        for rnd in range(rounds):
            for entry, call in calls.items():
                for on in (1, 0):
                    lib.frl_decoder_mse_bwd_subgroups(on)
                    call()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(8):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    res.setdefault(f"{name} {entry} {'subgroups' if on else 'lockstep'}", []).append(e0.elapsed_time(e1) * 125)
        lib.frl_decoder_mse_bwd_subgroups(1)
    return res


def report(res, label=""):
    for k, v in res.items():
        r = sorted(v)
        print(f"{label}{k:32s}", [round(x, 1) for x in r], "median", round(r[len(r) // 2], 1), "spread", round(r[-1] - r[0], 1), "us per call")


if __name__ == "__main__":
    if "--child" in sys.argv:
        print("RESULT " + json.dumps(measure(1)))
    elif "--tags" in sys.argv:
        tags = sys.argv[sys.argv.index("--tags") + 1].split(",")
        allres = {t: {} for t in tags}
        for rnd in range(ROUNDS):
            for t in tags:
                env = dict(os.environ)
                env.pop("FRL_HIP_LIB_TAG", None)
                if t:
                    env["FRL_HIP_LIB_TAG"] = t
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
                line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
                if out.returncode != 0 or not line:
                    sys.stderr.write(out.stdout + out.stderr)
                    sys.exit(f"library '{t}' failed (exit code {out.returncode})")
                for k, v in json.loads(line[0][7:]).items():
                    allres[t].setdefault(k, []).extend(v)
        for t in tags:
            report(allres[t], f"[{t or 'default'}] ")
        print("JSON " + json.dumps(allres))
    else:
        report(measure(ROUNDS))

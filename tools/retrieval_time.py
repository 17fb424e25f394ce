"""Times pero_sim_topk (k = 10, key splits on auto, cosine scales) against torch.topk(q @ keys.T, 10) on the same device and dtype, at the
evaluation batch (16384 x 16384 x 4096) and at the visualiser's shape (64 queries): everything warmed up, three alternating rounds of
device-event windows of about 0.4 s, one JSON line per shape.  FLOP and byte counts come from the shapes."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pero_pretraining_amd import ops  # noqa: E402

PEAK = {torch.float32: 157.3e12, torch.bfloat16: 2516.6e12}
HBM = 8.0e12


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    out = []
    k = 10
    for M, N, D, dtype in [(16384, 16384, 4096, torch.bfloat16), (64, 16384, 4096, torch.bfloat16), (16384, 16384, 4096, torch.float32),
                           (64, 16384, 4096, torch.float32)]:
        g = torch.Generator(device="cuda").manual_seed(M + N)
        q = torch.randn((M, D), device="cuda", generator=g).to(dtype)
        keys = torch.randn((N, D), device="cuda", generator=g).to(dtype)
        qs, ks = ops.inv_rownorm(q), ops.inv_rownorm(keys)

        def fused():
            return ops.sim_topk(q, keys, k, q_scale=qs, key_scale=ks)

        def dense():
            return torch.topk(q @ keys.T, k)

        def gemm_only():
            return q @ keys.T

        idx, val = fused()
        dv, di = dense()
        torch.cuda.synchronize()
        # same question, scores unscaled in the dense form: compare on the unscaled call
        idx0, _ = ops.sim_topk(q, keys, k)
        agree = float((idx0.long() == di).float().mean())
        one = timed(fused, 2)
        reps = max(3, min(200, int(400.0 / max(one, 0.01))))
        rounds = {"fused": [], "dense": [], "gemm_only": []}
        for _ in range(3):
            for name, fn in (("fused", fused), ("dense", dense), ("gemm_only", gemm_only)):
                rounds[name].append(timed(fn, reps))
        es = 4 if dtype == torch.float32 else 2
        flop = 2.0 * M * N * D
        splits = ops.sim_topk_key_splits(M, N)
        qt, kt = -(-M // 64), -(-N // 128)
        need = (M * D + N * D) * es + M * k * 8 + (M + N) * 4
        moved = (qt * N * D + kt * M * D) * es + M * k * 8 + (2 * splits * M * k * 8 if splits > 1 else 0)   # what the workgroups request
        best = min(rounds["fused"])
        floor = max(flop / PEAK[dtype], need / HBM)
        rec = {"M": M, "N": N, "D": D, "dtype": str(dtype), "k": k, "key_splits": splits, "reps": reps,
               "fused_ms": rounds["fused"], "dense_ms": rounds["dense"], "gemm_only_ms": rounds["gemm_only"],
               "fused_tflops": flop / best / 1e9, "mfma_peak_fraction": flop / best / 1e-3 / PEAK[dtype],
               "floor_ms": floor * 1e3, "share_of_floor": floor * 1e3 / best, "bytes_needed": need, "bytes_requested": moved,
               "dense_matrix_bytes": M * N * es, "idx_agreement_with_dense": agree}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        del q, keys
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

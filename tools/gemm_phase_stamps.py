"""In-kernel phase stamps of the big-tile expert GEMMs at the benchmark shape.

Builds the library with -DFM_GEMM_STAMPS into a scratch path (or takes a
prebuilt one with --lib), runs the bench.py workload (S=4096 H=1024
P=4096 E=8 top-2 bf16) and prints, per GEMM phase, the medians over all
(block, job) records of

  prologue  = first MFMA  - job entry
  main loop = end K-loop  - first MFMA
  epilogue  = end epilogue - end K-loop   (store issue; no drain wait)

in microseconds (100 MHz wall clock, 10 ns resolution), split by the
block's 1st/2nd/... job of the persistent walk. The stamped build is a
measurement build: the default library contains no stamp code.

Usage: python tools/gemm_phase_stamps.py [--lib PATH] [--steps N]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PHASE_NAMES = {0: "up (PHASE 0)", 1: "down (PHASE 1)", 2: "packed (PHASE 2)",
               3: "logits (PHASE 3)"}
SHAPE = (4, 512, 4, 4)  # phases, blocks, jobs, stamps (mirrors the kernel)


def build_stamped(path):
    src = os.path.join(REPO, "flashmoe_amd", "csrc", "flashmoe_kernels.hip")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared",
           "-fPIC", "-DFM_GEMM_STAMPS", src, "-o", path]
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, cwd=REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None,
                    help="prebuilt -DFM_GEMM_STAMPS library (default: build "
                         "one into a temporary directory)")
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()

    lib_path = args.lib
    if lib_path is None:
        lib_path = os.path.join(tempfile.mkdtemp(prefix="fm_stamps_"),
                                "_libflashmoe_stamps.so")
        build_stamped(lib_path)

    import numpy as np
    import torch

    import flashmoe_amd._ext as _ext

    _ext._LIB_PATH = os.path.abspath(lib_path)
    from flashmoe_amd import moe

    lib = _ext.load()
    lib.fm_debug_gemm_stamps.argtypes = [ctypes.c_void_p]
    lib.fm_debug_gemm_stamps.restype = ctypes.c_int

    S, H, P, E = 4096, 1024, 4096, 8
    cfg = {"capacity_factor": 1, "drop_tokens": 1, "expert_top_k": 2,
           "global_batch": 256, "is_training": 0, "hidden_act": 0,
           "hidden_size": H, "intermediate_size": P, "mini_batch": 1,
           "moe_frequency": 1, "num_experts": E, "num_layers": 1,
           "sequence_len": S, "torch_dtype": 2, "vocab_size": 32000}
    with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
        json.dump(cfg, f)
    moe.initialize(f.name, rank=0, world_size=1)
    torch.manual_seed(47)
    x = torch.randn(1, S, H, dtype=torch.bfloat16, device="cuda")
    gw = torch.randn(H, E, dtype=torch.bfloat16, device="cuda")
    ew = torch.randn(E, 2, P, H, dtype=torch.bfloat16, device="cuda")

    buf = np.zeros(SHAPE, dtype=np.uint64)
    for _ in range(5):
        moe.moe_forward(x, gw, ew)
    _ext.check(lib.fm_debug_gemm_stamps(ctypes.c_void_p(buf.ctypes.data)),
               "fm_debug_gemm_stamps")
    recs = []  # one [phases, blocks, jobs, 4] array per forward
    for _ in range(args.steps):
        moe.moe_forward(x, gw, ew)
        _ext.check(lib.fm_debug_gemm_stamps(ctypes.c_void_p(buf.ctypes.data)),
                   "fm_debug_gemm_stamps")
        recs.append(buf.astype(np.int64))
    moe.finalize()
    r = np.stack(recs)  # [steps, phases, blocks, jobs, 4]

    print(f"gemm phase stamps: S={S} H={H} P={P} E={E} top-2 bf16, "
          f"{args.steps} forwards, medians in us over (forward, block)")
    print(f"{'kernel':18s} {'job':>3s} {'records':>8s} {'prologue':>9s} "
          f"{'mainloop':>9s} {'epilogue':>9s} {'total':>8s}")
    for ph in range(SHAPE[0]):
        tot = {"pro": 0.0, "main": 0.0, "epi": 0.0}
        any_rec = False
        for j in range(SHAPE[2]):
            s = r[:, ph, :, j, :].reshape(-1, 4)
            s = s[s[:, 0] > 0]
            if len(s) == 0:
                continue
            any_rec = True
            pro = np.median(s[:, 1] - s[:, 0]) / 100.0
            mainl = np.median(s[:, 2] - s[:, 1]) / 100.0
            epi = np.median(s[:, 3] - s[:, 2]) / 100.0
            tot["pro"] += pro
            tot["main"] += mainl
            tot["epi"] += epi
            print(f"{PHASE_NAMES[ph]:18s} {j:3d} {len(s):8d} {pro:9.2f} "
                  f"{mainl:9.2f} {epi:9.2f} {pro + mainl + epi:8.2f}")
        if any_rec:
            # gap between a block's consecutive jobs (epilogue end of job j
            # to entry of job j+1), where the walk has more than one
            s0 = r[:, ph, :, 0, :].reshape(-1, 4)
            s1 = r[:, ph, :, 1, :].reshape(-1, 4)
            both = (s0[:, 0] > 0) & (s1[:, 0] > 0)
            gap = (np.median(s1[both, 0] - s0[both, 3]) / 100.0
                   if both.any() else float("nan"))
            t = tot["pro"] + tot["main"] + tot["epi"]
            print(f"{PHASE_NAMES[ph]:18s} sum {'':8s} {tot['pro']:9.2f} "
                  f"{tot['main']:9.2f} {tot['epi']:9.2f} {t:8.2f}   "
                  f"(prologue+epilogue = "
                  f"{100.0 * (tot['pro'] + tot['epi']) / t:.1f}% of the "
                  f"block's walk; job0->job1 gap {gap:.2f})")


if __name__ == "__main__":
    main()

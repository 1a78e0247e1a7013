"""In-kernel phase stamps of the big-tile expert GEMMs at the benchmark shape.

Builds the library with -DFM_GEMM_STAMPS into a scratch path (or takes a
prebuilt one with --lib), runs the bench.py workload (S=4096 H=1024
P=4096 E=8 top-2 bf16) and prints, per GEMM phase, the medians over all
(block, job) records of

  prologue  = first MFMA  - job entry
  main loop = end K-loop  - first MFMA
  epilogue  = end epilogue - end K-loop   (store issue; no drain wait)

in microseconds (100 MHz wall clock, 10 ns resolution), split by the
block's 1st/2nd/... job of the persistent walk.

Before that table it prints a timeline of the forward. The stamps are
absolute values of one clock common to the chip, and thread 0 of every
k_gate_fused / k_cast_combine block records its entry and exit too, so
per forward (medians over forwards) the tool lays out

  - first block entry, last block exit and span of each of the four
    kernels, relative to the gate's first entry, and the dead time at
    each seam (last exit of one kernel to first entry of the next);
  - for both GEMMs: p50/p95/max of a block's walk (first entry to last
    stamp), of its entry skew (entry - kernel's first entry) and of its
    idle tail (kernel's last stamp - block's last stamp), and the median
    walk per linear block id % 8 (the XCD a block lands on);
  - the wall time per forward of the same stamped build (back-to-back
    forwards between two events) next to the sum of spans and seams.

A GEMM block's last stamp is the end of its epilogue's store ISSUE; the
drain of those stores shows up in the seam after the kernel. The stamped
build is a measurement build: the default library contains no stamp code.

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
AUX_SHAPE = (2, 4096, 2)  # gate / combine, blocks, entry / exit
TICKS_PER_US = 100.0


def _pct(v, qs):
    import numpy as np
    return [float(np.percentile(v, q)) / TICKS_PER_US for q in qs]


def forward_timeline(gemm, aux):
    """One forward's stamps -> dict of figures in us (None: a kernel left no
    record). gemm: [phases, blocks, jobs, 4], aux: [2, blocks, 2], int64."""
    import numpy as np

    def aux_blocks(k):
        a = aux[k]
        a = a[(a[:, 0] > 0) & (a[:, 1] > 0)]
        return a[:, 0], a[:, 1], None

    def gemm_blocks(ph):
        g = gemm[ph]                              # [blocks, jobs, 4]
        ran = g[:, :, 0] > 0                      # [blocks, jobs]
        has = ran.any(axis=1)
        big = np.iinfo(np.int64).max
        first = np.where(ran, g[:, :, 0], big).min(axis=1)[has]
        last = np.where(ran, g[:, :, 3], 0).max(axis=1)[has]
        return first, last, np.nonzero(has)[0]

    kernels = [("gate", aux_blocks(0)), ("up", gemm_blocks(0)),
               ("down", gemm_blocks(1)), ("combine", aux_blocks(1))]
    if any(len(k[1][0]) == 0 for k in kernels):
        return None
    t0 = kernels[0][1][0].min()
    out = {}
    prev_end = None
    for name, (first, last, ids) in kernels:
        k0, k1 = first.min(), last.max()
        out[name + ".first"] = (k0 - t0) / TICKS_PER_US
        out[name + ".last"] = (k1 - t0) / TICKS_PER_US
        out[name + ".span"] = (k1 - k0) / TICKS_PER_US
        if prev_end is not None:
            out[name + ".dead_before"] = (k0 - prev_end) / TICKS_PER_US
        prev_end = k1
        if ids is None:
            continue
        for key, v in (("walk", last - first), ("skew", first - k0),
                       ("tail", k1 - last)):
            p50, p95, mx = _pct(v, (50, 95, 100))
            out[f"{name}.{key}.p50"] = p50
            out[f"{name}.{key}.p95"] = p95
            out[f"{name}.{key}.max"] = mx
        for x in range(8):
            w = (last - first)[ids % 8 == x]
            out[f"{name}.walk.xcd{x}"] = (
                float(np.median(w)) / TICKS_PER_US if len(w) else float("nan"))
    out["total"] = (prev_end - t0) / TICKS_PER_US
    return out


def print_timeline(tls, wall_us):
    import numpy as np

    def med(key):
        return float(np.median([t[key] for t in tls]))

    print(f"timeline of the forward: medians over {len(tls)} forwards, us, "
          "relative to the gate's first block entry")
    print(f"{'kernel':10s} {'dead before':>11s} {'first entry':>11s} "
          f"{'last exit':>10s} {'span':>8s}")
    acc = 0.0
    for name in ("gate", "up", "down", "combine"):
        dead = med(name + ".dead_before") if name != "gate" else 0.0
        acc += dead + med(name + ".span")
        print(f"{name:10s} {dead:11.2f} {med(name + '.first'):11.2f} "
              f"{med(name + '.last'):10.2f} {med(name + '.span'):8.2f}")
    print(f"sum of spans and dead times {acc:.2f}; first entry to last exit "
          f"{med('total'):.2f}; wall per forward {wall_us:.2f} "
          f"(back-to-back forwards of this stamped build)")
    print(f"{'GEMM':6s} {'figure':22s} {'p50':>8s} {'p95':>8s} {'max':>8s}")
    for name in ("up", "down"):
        for key, label in (("walk", "block walk"),
                           ("skew", "entry - first entry"),
                           ("tail", "idle after last stamp")):
            print(f"{name:6s} {label:22s} {med(f'{name}.{key}.p50'):8.2f} "
                  f"{med(f'{name}.{key}.p95'):8.2f} "
                  f"{med(f'{name}.{key}.max'):8.2f}")
        print(f"{name:6s} median walk by block id % 8: " + " ".join(
            f"{med(f'{name}.walk.xcd{x}'):.2f}" for x in range(8)))
    print()


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
    lib.fm_debug_aux_stamps.argtypes = [ctypes.c_void_p]
    lib.fm_debug_aux_stamps.restype = ctypes.c_int

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
    abuf = np.zeros(AUX_SHAPE, dtype=np.uint64)

    def read_stamps():
        _ext.check(lib.fm_debug_gemm_stamps(ctypes.c_void_p(buf.ctypes.data)),
                   "fm_debug_gemm_stamps")
        _ext.check(lib.fm_debug_aux_stamps(ctypes.c_void_p(abuf.ctypes.data)),
                   "fm_debug_aux_stamps")

    for _ in range(5):
        moe.moe_forward(x, gw, ew)
    read_stamps()
    recs = []  # one [phases, blocks, jobs, 4] array per forward
    tls = []   # one timeline dict per forward
    for _ in range(args.steps):
        moe.moe_forward(x, gw, ew)
        read_stamps()
        recs.append(buf.astype(np.int64))
        tl = forward_timeline(recs[-1], abuf.astype(np.int64))
        if tl is not None:
            tls.append(tl)
    # wall time of the same build: back-to-back forwards between two events
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    nwall = 50
    ev0.record()
    for _ in range(nwall):
        moe.moe_forward(x, gw, ew)
    ev1.record()
    torch.cuda.synchronize()
    wall_us = ev0.elapsed_time(ev1) * 1000.0 / nwall
    read_stamps()
    moe.finalize()
    r = np.stack(recs)  # [steps, phases, blocks, jobs, 4]

    if tls:
        print_timeline(tls, wall_us)
    else:
        print("timeline: a kernel of the forward left no stamps "
              "(not the four-kernel classic path?)")

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

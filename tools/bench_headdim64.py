"""head_dim-64 decode at Llama-3.2-1B geometry: 16 layers, 32 q / 8 kv heads, D = 64, batch 8, K / V sparsity 70 %.

Prints ONE JSON line.  Per cache length L (prefill of L tokens, then decode):
  tok_s             decode tokens/s: a captured graph of one step over all layers (decode_fused with a step counter), replayed;
                    device-event time of the replays, windows reset every 16 steps (the trigger is not part of the step)
  kernel_us         mean device time of one layer's decode launch (mustafar_profile_*: the "key" record), finish_us the row merge
  bytes_per_layer   bytes the step must read per layer: compressed K / V streams + bitmaps + offsets, dense window rows, q and out
  frac_8tbs_kernel  bytes_per_layer / kernel_us over 8 TB/s;  frac_8tbs_step  16 x bytes_per_layer per step over 8 TB/s
and, at L = 8192, prune_convert_us_per_layer: device-synchronised wall time of one layer's prefill prune + two-pass conversion of K and V.
--generate N (with --gen-length L, default 8192; default N = 0: leg off) adds a generate leg: N tokens from a prefill of L (600 tokens: three
triggers), timed two ways, alternated A B A B in one process:
  extents   MustafarConfig(hd64_extents=True): ONE captured graph of the step with a device-side T, replayed through every trigger;
            the trigger step runs eagerly for all layers (decode_fused(defer_trigger=True) + run_triggers: one batched call)
  tuple     the parent's way: the tuple cache, the trigger inside the eager step, every array moved, so the graph is captured again
Each reports tok_s over the whole generate (host wall time, device-synchronised at the end) and trigger_step_ms, the mean wall time of a
step that fires a trigger (recapture included for the tuple way); and ext_kernel_us / plain_kernel_us: the decode launch of the EXT
instantiation against the plain one at the same T with no extent listed.
--prefill (default off; --prefill-runs N, default 21) adds a prefill leg at L = 8192, one layer, alternated A B A B in one process behind
a warm-up of 3 runs each, median wall time of N runs per way, every run ended by a device synchronise:
  prefill_old_us    the parent's route: prune + two conversions of K and V (build_cache; its host waits included)
  prefill_raw_us    MustafarConfig(hd64_raw_prefill=True): cache64.compress_raw_pair_hd64 (its one wait included) + the windows
and consolidate() of one side at a base of 7936 tokens plus 3 and plus 32 extents, on the device and through to_reference(), the same way.
The results of both ways are compared bit for bit before anything is timed.
Needs an MI355X; it does not fall back to anything.  Usage: python tools/bench_headdim64.py [--lengths 4096,8192,32768] [--steps 64]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctypes  # noqa: E402

import torch  # noqa: E402

from mustafar_amd import _lib  # noqa: E402
from mustafar_amd.hook import MustafarAttention, MustafarConfig  # noqa: E402

LAYERS, HQ, HKV, D, BATCH, S = 16, 32, 8, 64, 8, 0.7


def stream_bytes(c) -> int:
    bmp, idx, nzs, off = c
    return bmp.numel() * 8 + idx.numel() * 4 + nzs.flat.numel() * 2 + off.numel() * 4


def run_length(L: int, steps: int, dev) -> dict:
    attn = MustafarAttention(MustafarConfig(num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D, k_sparsity=S, v_sparsity=S,
                                            api="fused"))
    g = torch.Generator(device=dev).manual_seed(L)
    pasts, conv_us = [], []
    for layer in range(LAYERS):
        K = torch.randn((BATCH, HKV, L, D), generator=g, device=dev).half()
        V = torch.randn((BATCH, HKV, L, D), generator=g, device=dev).half()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        past = attn.build_cache(K, V)
        torch.cuda.synchronize()
        conv_us.append((time.perf_counter() - t0) * 1e6)
        pasts.append(attn.to_fused(past))
        del K, V
    C, wl = pasts[0][4], pasts[0][1].len
    win_bytes = BATCH * HKV * (wl + 1) * D * 2 * 2
    per_layer = stream_bytes(pasts[0][0]) + stream_bytes(pasts[0][2]) + win_bytes + 2 * BATCH * HQ * D * 2
    q = torch.randn((BATCH, HQ, 1, D), generator=g, device=dev).half()
    kn = torch.randn((BATCH, HKV, 1, D), generator=g, device=dev).half()
    vn = torch.randn((BATCH, HKV, 1, D), generator=g, device=dev).half()
    ctr = torch.zeros((1,), dtype=torch.int32, device=dev)
    Lb = _lib.load()

    def step():
        for p in pasts:
            attn.decode_fused(q, kn, vn, p, step_counter=ctr)
        Lb.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, ctr.data_ptr(), 1)

    def reset():
        ctr.zero_()

    # ---- kernel time (profile records; eager calls, one record per layer call)
    for _ in range(2):
        step()
    reset()
    torch.cuda.synchronize()
    n_rec = 4 * LAYERS
    _lib.check(Lb.mustafar_profile_begin(n_rec), "mustafar_profile_begin")
    for _ in range(4):
        step()
    reset()
    k_us, v_us, f_us, recs = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _lib.check(Lb.mustafar_profile_end2(ctypes.byref(k_us), ctypes.byref(v_us), ctypes.byref(f_us), ctypes.byref(recs)), "mustafar_profile_end2")
    assert Lb.mustafar_last_decode_choice() == (1 << 4) | (5 << 8)
    # ---- tokens/s: graph replays of one step over all layers
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    reset()
    room = pasts[0][1].cap - wl - 1   # steps before the windows are full
    per_round = max(1, min(16, room))
    for _ in range(per_round):       # warm-up
        graph.replay()
    reset()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total_ms, done = 0.0, 0
    while done < steps:
        n = min(per_round, steps - done)
        ev0.record()
        for _ in range(n):
            graph.replay()
        ev1.record()
        ev1.synchronize()
        total_ms += ev0.elapsed_time(ev1)
        done += n
        reset()
    step_us = total_ms * 1e3 / done
    torch.cuda.synchronize()
    return {"L": L, "compressed": C, "window": wl + 1, "tok_s": round(BATCH * 1e6 / step_us, 1), "step_us": round(step_us, 2),
            "kernel_us": round(k_us.value, 3), "finish_us": round(f_us.value, 3), "records": recs.value,
            "bytes_per_layer": per_layer, "frac_8tbs_kernel": round(per_layer / (k_us.value * 1e-6) / 8e12, 4),
            "frac_8tbs_step": round(LAYERS * per_layer / (step_us * 1e-6) / 8e12, 4),
            "prune_convert_us_per_layer": round(sorted(conv_us[1:])[len(conv_us[1:]) // 2], 1)}


def _kernel_us(Lb, fn, n=4):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    _lib.check(Lb.mustafar_profile_begin(n * LAYERS), "mustafar_profile_begin")
    for _ in range(n):
        fn()
    k_us, v_us, f_us, recs = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _lib.check(Lb.mustafar_profile_end2(ctypes.byref(k_us), ctypes.byref(v_us), ctypes.byref(f_us), ctypes.byref(recs)), "mustafar_profile_end2")
    return k_us.value


def generate(L: int, n_tokens: int, extents: bool, dev, kernel_ab: bool = False) -> dict:
    """One generate of n_tokens from a prefill of L tokens (the same random data for both ways)."""
    R = 32
    attn = MustafarAttention(MustafarConfig(num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D, k_sparsity=S, v_sparsity=S,
                                            api="fused", residual_length=R, hd64_extents=extents))
    g = torch.Generator(device=dev).manual_seed(L + 1)
    pasts = []
    for layer in range(LAYERS):
        K = torch.randn((BATCH, HKV, L, D), generator=g, device=dev).half()
        V = torch.randn((BATCH, HKV, L, D), generator=g, device=dev).half()
        pasts.append(attn.to_fused(attn.build_cache(K, V)))
        del K, V
    q = torch.randn((BATCH, HQ, 1, D), generator=g, device=dev).half()
    kn = torch.randn((BATCH, HKV, 1, D), generator=g, device=dev).half()
    vn = torch.randn((BATCH, HKV, 1, D), generator=g, device=dev).half()
    ctr = torch.zeros((1,), dtype=torch.int32, device=dev)
    Lb = _lib.load()
    C0 = pasts[0][4]
    n_trig = sum(1 for i in range(n_tokens) if (L + i + 1 - R - C0) % 256 == 0)
    cap = C0 + 256 * max(1, n_trig)
    t_dev = torch.tensor([C0], dtype=torch.int32, device=dev)
    kw = dict(step_counter=ctr, t_device=t_dev, t_capacity=cap) if extents else dict(step_counter=ctr)
    res = {}
    if kernel_ab and extents:   # the EXT instantiation with no extent listed against the plain launch, same T
        res["plain_kernel_us"] = round(_kernel_us(Lb, lambda: [attn.decode_fused(q, kn, vn, p, step_counter=ctr) for p in pasts]), 3)
        assert Lb.mustafar_last_decode_choice() >> 8 == 5
        t_dev.fill_(C0)
        ab = dict(step_counter=ctr, t_device=t_dev, t_capacity=C0 + 256)
        res["ext_kernel_us"] = round(_kernel_us(Lb, lambda: [attn.decode_fused(q, kn, vn, p, **ab) for p in pasts]), 3)
        assert Lb.mustafar_last_decode_choice() >> 8 == 6
        res["kernel_T"] = C0

    def capture():
        ctr.zero_()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for p in pasts:
                attn.decode_fused(q, kn, vn, p, **kw)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for p in pasts:
                attn.decode_fused(q, kn, vn, p, **kw)
            Lb.mustafar_counter_add(torch.cuda.current_stream().cuda_stream, ctr.data_ptr(), 1)
        return graph

    graph = capture()
    torch.cuda.synchronize()
    since, trig_ms = 0, []
    t_start = time.perf_counter()
    for i in range(n_tokens):
        n = pasts[0][5] + since + 1
        if (n - R - pasts[0][4]) % 256 == 0 and pasts[0][1].len + since + 1 >= 256:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pasts = [attn.advance(p, since) for p in pasts]
            since = 0
            if extents:   # the step eagerly, then the trigger of all layers in one batched call; the graph lives on
                pasts = [attn.decode_fused(q, kn, vn, p, defer_trigger=True)[1] for p in pasts]
                pasts = attn.run_triggers(pasts)
                t_dev.add_(256)
                ctr.add_(1 - 256)
            else:         # the step with its trigger inside, then a new capture: every array has moved
                pasts = [attn.decode_fused(q, kn, vn, p)[1] for p in pasts]
                graph = capture()
            torch.cuda.synchronize()
            trig_ms.append((time.perf_counter() - t0) * 1e3)
        else:
            graph.replay()
            since += 1
    torch.cuda.synchronize()
    wall = time.perf_counter() - t_start
    res.update({"way": "extents" if extents else "tuple", "tok_s": round(BATCH * n_tokens / wall, 1), "triggers": len(trig_ms),
                "trigger_step_ms": round(sum(trig_ms) / max(1, len(trig_ms)), 3)})
    return res


def _same_cache(a, b) -> bool:
    return torch.equal(a[0].reshape(-1), b[0].reshape(-1)) and torch.equal(a[1].reshape(-1), b[1].reshape(-1)) and torch.equal(a[3], b[3]) and \
        torch.equal(a[2].flat.view(torch.int16), b[2].flat.view(torch.int16))


def _ab_median_us(fa, fb, runs: int, warm: int = 3):
    """Median wall time (us) of fa and fb, alternated A B A B behind `warm` runs of each; every run ends in a device synchronise."""
    def once(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6
    for _ in range(warm):
        once(fa)
        once(fb)
    ta, tb = [], []
    for _ in range(runs):
        ta.append(once(fa))
        tb.append(once(fb))
    return sorted(ta)[runs // 2], sorted(tb)[runs // 2]


def prefill_leg(dev, runs: int) -> dict:
    from mustafar_amd.cache64 import ExtentCache64
    from mustafar_amd.compression import kth_from_sparsity
    L, R = 8192, 32
    cfg = dict(num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D, k_sparsity=S, v_sparsity=S, api="fused", residual_length=R)
    old, raw = MustafarAttention(MustafarConfig(**cfg)), MustafarAttention(MustafarConfig(hd64_raw_prefill=True, **cfg))
    g = torch.Generator(device=dev).manual_seed(8192)
    K = torch.randn((BATCH, HKV, L, D), generator=g, device=dev).half()
    V = torch.randn((BATCH, HKV, L, D), generator=g, device=dev).half()
    po, pr = old.build_cache(K, V), raw.build_cache(K, V)
    assert po[4] == pr[4] == 7936 and _same_cache(po[0], pr[0]) and _same_cache(po[2], pr[2]), "the two prefill routes disagree"
    assert torch.equal(po[1], pr[1]) and torch.equal(po[3], pr[3])
    del po, pr
    t_old, t_raw = _ab_median_us(lambda: old.build_cache(K, V), lambda: raw.build_cache(K, V), runs)
    res = {"L": L, "runs": runs, "prefill_old_us": round(t_old, 1), "prefill_raw_us": round(t_raw, 1), "prefill_old_over_raw": round(t_old / t_raw, 3)}
    kth = kth_from_sparsity(S, D)
    Bp = BATCH * HKV
    for n_ext in (3, 32):
        past = raw.build_cache(K[:, :, :7936 + R].contiguous(), V[:, :, :7936 + R].contiguous())
        kc, vc = ExtentCache64(past[0], "key", Bp, 7936), ExtentCache64(past[2], "value", Bp, 7936)
        for i in range(n_ext):
            kb = torch.randn((BATCH, HKV, 256 + R, D), generator=g, device=dev).half()
            vb = torch.randn((BATCH, HKV, 256 + R, D), generator=g, device=dev).half()
            ExtentCache64.append_extents([(kc, vc)], [(kb, vb)], kth, kth, 256 + R)
        a, b = kc.consolidate(), kc.consolidate(via_reference=True)
        assert a.tokens == b.tokens == 7936 + 256 * n_ext and _same_cache(a.base, b.base), "the two consolidations disagree"
        del a, b
        t_dev, t_ref = _ab_median_us(lambda: kc.consolidate(), lambda: kc.consolidate(via_reference=True), runs)
        res[f"consolidate_{n_ext}_device_us"] = round(t_dev, 1)
        res[f"consolidate_{n_ext}_reference_us"] = round(t_ref, 1)
        del kc, vc, past
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="4096,8192,32768")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--generate", type=int, default=0)
    ap.add_argument("--gen-length", type=int, default=8192)
    ap.add_argument("--prefill", action="store_true")
    ap.add_argument("--prefill-runs", type=int, default=21)
    args = ap.parse_args()
    if args.prefill_runs < 20:
        raise SystemExit("--prefill-runs: at least 20 runs per way")
    if not torch.cuda.is_available():
        raise SystemExit("bench_headdim64 needs a GPU")
    dev = torch.device("cuda:0")
    res = []
    for L in (int(v) for v in args.lengths.split(",") if v):
        res.append(run_length(L, args.steps, dev))
        torch.cuda.empty_cache()
    out = {"workload": "llama-3.2-1b decode, head_dim 64", "layers": LAYERS, "q_heads": HQ, "kv_heads": HKV, "head_dim": D, "batch": BATCH,
           "k_sparsity": S, "v_sparsity": S, "device": torch.cuda.get_device_name(dev), "results": res,
           "prune_convert_us_per_layer_L8192": next((r["prune_convert_us_per_layer"] for r in res if r["L"] == 8192), None)}
    if args.generate > 0:   # A B A B: extents, tuple, extents, tuple
        runs = []
        for rep in range(2):
            for ext in (True, False):
                runs.append(generate(args.gen_length, args.generate, ext, dev, kernel_ab=rep == 0))
                torch.cuda.empty_cache()
        out["generate"] = {"L": args.gen_length, "tokens": args.generate, "runs": runs}
    if args.prefill:
        out["prefill"] = prefill_leg(dev, args.prefill_runs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

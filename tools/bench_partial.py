"""What the LSE and a split step cost, one layer, at the headline shape (Llama-3-8B heads, D = 128, L = 8192, batch 8, arena)
and at Llama-3.2-1B geometry (32 q / 8 kv heads, D = 64, L = 8192, batch 8, tuple cache).  Prints ONE JSON line; per shape:
  finish_us / finish_lse_us   mean device time of the row kernel behind the one-pass launch without and with the LSE store
                              (mustafar_profile_end2, eager calls, alternated A B A B)
  merge2_us                   mustafar_merge_attention_states for 2 parts: a captured graph of --merges launches back to back, device
                              events around its replays, per launch (kernel + the gap to the next launch)
  fused_step_us               one decode_fused step over the whole cache: a captured graph of the step, device events around --steps replays
  split_step_us               one decode_split step: the first half of the compressed tokens as a frozen segment (one window-less call),
                              decode_fused(return_lse=True) over the rest, one merge -- captured and timed the same way, alternated with the above
Needs an MI355X; it does not fall back to anything.  Usage: python tools/bench_partial.py [--steps 200] [--merges 100] [--records 64]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mustafar_amd import _lib  # noqa: E402
from mustafar_amd.hook import MustafarAttention, MustafarConfig  # noqa: E402

SHAPES = {  # name: (Hq, Hkv, D, L, batch, hook options)
    "headline_c3": (32, 8, 128, 8192, 8, {"arena": True}),
    "llama_3_2_1b": (32, 8, 64, 8192, 8, {}),
}
S = 0.7


def fork(past):
    return (past[0], past[1].clone(), past[2], past[3].clone(), past[4], past[5])


def finish_us(Lb, attn, q, kn, vn, past, records, with_lse):
    ctr = torch.zeros((1,), dtype=torch.int32, device=q.device)   # (a step counter of zero: the host-side window length does not advance)
    _lib.check(Lb.mustafar_profile_begin(records), "mustafar_profile_begin")
    for _ in range(records):
        attn.decode_fused(q, kn, vn, past, step_counter=ctr, return_lse=with_lse)
    torch.cuda.synchronize()
    k, v, f, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _lib.check(Lb.mustafar_profile_end2(ctypes.byref(k), ctypes.byref(v), ctypes.byref(f), ctypes.byref(n)), "mustafar_profile_end2")
    assert n.value == records
    return f.value


def graph_of(fn, warm=2):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def replay_us(g, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def run(name, a, dev):
    Hq, Hkv, D, L, B, kw = SHAPES[name]
    Lb = _lib.load()
    attn = MustafarAttention(MustafarConfig(num_attention_heads=Hq, num_key_value_heads=Hkv, head_dim=D, k_sparsity=S, v_sparsity=S, api="fused", **kw))
    g = torch.Generator(device=dev).manual_seed(L + D)
    K = torch.randn((B, Hkv, L, D), generator=g, device=dev).half()
    V = torch.randn((B, Hkv, L, D), generator=g, device=dev).half()
    q = torch.randn((B, Hq, 1, D), generator=g, device=dev).half()
    kn = torch.randn((B, Hkv, 1, D), generator=g, device=dev).half()
    vn = torch.randn((B, Hkv, 1, D), generator=g, device=dev).half()
    whole = attn.to_fused(attn.build_cache(K, V))
    C = whole[4]
    F = C // 2 // 256 * 256
    R = attn.cfg.residual_length
    seg = attn.build_cache(K[:, :, :F + R].contiguous(), V[:, :, :F + R].contiguous())   # its first F tokens, compressed: the frozen segment
    assert seg[4] == F
    frozen = [(seg[0], seg[2], F)]
    live = attn.to_fused(attn.build_cache(K[:, :, F:].contiguous(), V[:, :, F:].contiguous()))
    assert live[4] == C - F
    del K, V
    out = {"compressed_tokens": C, "frozen_tokens": F}
    # ---- the row kernel without / with the LSE
    for _ in range(2):
        finish_us(Lb, attn, q, kn, vn, fork(whole), 8, False)
        finish_us(Lb, attn, q, kn, vn, fork(whole), 8, True)
    fa, fb = [], []
    for _ in range(4):
        fa.append(finish_us(Lb, attn, q, kn, vn, fork(whole), a.records, False))
        fb.append(finish_us(Lb, attn, q, kn, vn, fork(whole), a.records, True))
    out["finish_us"], out["finish_lse_us"] = round(sum(fa) / 4, 3), round(sum(fb) / 4, 3)
    out["finish_us_runs"], out["finish_lse_us_runs"] = [round(x, 3) for x in fa], [round(x, 3) for x in fb]
    # ---- the merge of 2 parts
    BH = B * Hq
    parts = torch.randn((2, BH, D), generator=g, device=dev).half()
    lses = torch.randn((2, BH), generator=g, device=dev).float() * 3
    mo = torch.empty((BH, D), dtype=torch.float16, device=dev)
    ml = torch.empty((BH,), dtype=torch.float32, device=dev)

    def merges():
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(a.merges):
            _lib.check(Lb.mustafar_merge_attention_states(st, parts.data_ptr(), BH * D, lses.data_ptr(), BH, 2, BH, D, mo.data_ptr(), ml.data_ptr()),
                       "mustafar_merge_attention_states")

    gm = graph_of(merges)
    replay_us(gm, 5)
    out["merge2_us"] = round(min(replay_us(gm, 20) for _ in range(3)) / a.merges, 3)
    # ---- one fused step over the whole cache against one split step
    p_whole, p_live = fork(whole), fork(live)
    # (eager-form calls: each advances the host-side window length by one row -- three rows per graph, the same for both)
    g_fused = graph_of(lambda: attn.decode_fused(q, kn, vn, p_whole))
    g_split = graph_of(lambda: attn.decode_split(q, kn, vn, p_live, frozen))
    replay_us(g_fused, 20)
    replay_us(g_split, 20)
    ta, tb = [], []
    for _ in range(4):
        ta.append(replay_us(g_fused, a.steps))
        tb.append(replay_us(g_split, a.steps))
    out["fused_step_us"], out["split_step_us"] = round(sum(ta) / 4, 2), round(sum(tb) / 4, 2)
    out["fused_step_us_runs"], out["split_step_us_runs"] = [round(x, 2) for x in ta], [round(x, 2) for x in tb]
    # the two steps compute the same attention: compared before the numbers are reported
    o1, _ = attn.decode_fused(q, kn, vn, fork(p_whole))
    o2, _ = attn.decode_split(q, kn, vn, fork(p_live), frozen)
    out["split_vs_fused_max_abs"] = float((o1.float() - o2.float()).abs().max())
    assert out["split_vs_fused_max_abs"] < 2e-3, out
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--merges", type=int, default=100)
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_partial.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {"tool": "bench_partial", "device": torch.cuda.get_device_name(0)}
    for name in a.shapes.split(","):
        res[name] = run(name, a, dev)
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

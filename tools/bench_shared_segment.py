"""What one shared copy of a frozen segment saves: one layer, 32 q / 8 kv heads (G = 4), 7936 compressed tokens, at
head_dim 128 and 64, for 1, 2, 8 and 16 sequences that share the segment.  Two ways to the same attention:
  shared       partial.decode_segment over a SharedSegment: mustafar_decode_shared_segment + its row kernel, ONE copy of 8 heads
  replicated   partial.decode_segment over the same tokens held once per sequence (n_seqs x 8 heads): the route without this entry point
               (an arena at head_dim 128, the reference-layout arrays at head_dim 64)
Each way is a captured graph of --launches calls back to back, timed with device events around --replays replays behind warm-up
replays, the two alternated A B A B in one process; the outputs are compared before anything is timed.  Prints ONE JSON line: per head
dim and n_seqs the microseconds per call of both ways (mean of the rounds, and every round) and the bytes each way holds.
Needs an MI355X; it does not fall back to anything.  Usage: python tools/bench_shared_segment.py [--launches 20] [--replays 20] [--rounds 4]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mustafar_amd import partial  # noqa: E402
from mustafar_amd.cache import CompressedArena  # noqa: E402
from mustafar_amd.hook import MustafarAttention, MustafarConfig, _compress  # noqa: E402

HQ, HKV, T, S = 32, 8, 7936, 0.7


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


def held(c):
    if isinstance(c, CompressedArena):
        return c.bytes_in_use()
    return c[0].numel() * 8 + c[1].numel() * 4 + c[3].numel() * 4 + c[2].flat.numel() * 2


def run(D, n, a, dev):
    attn = MustafarAttention(MustafarConfig(num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D, k_sparsity=S, v_sparsity=S,
                                            api="fused", arena=(D == 128)))
    g = torch.Generator(device=dev).manual_seed(D + n)
    K = torch.randn((1, HKV, T, D), generator=g, device=dev).half()
    V = torch.randn((1, HKV, T, D), generator=g, device=dev).half()
    q = torch.randn((n, HQ, 1, D), generator=g, device=dev).half()
    seg = partial.SharedSegment.from_dense(attn, K, V)
    Kp = attn.dh_prune_key(K).expand(n, -1, -1, -1).reshape(n * HKV, T, D).contiguous()
    Vp = attn.dh_prune_value(V).expand(n, -1, -1, -1).reshape(n * HKV, T, D).contiguous()
    kc, vc = _compress(Kp, "key"), _compress(Vp, "value")
    del K, V, Kp, Vp
    if D == 128:
        kc, vc = CompressedArena.from_reference(kc, "key", T, None, 0.0), CompressedArena.from_reference(vc, "value", T, None, 0.0)
    shared = lambda: partial.decode_segment(attn, q, seg)
    replicated = lambda: partial.decode_segment(attn, q, kc, vc, T)
    (o1, l1), (o2, l2) = shared(), replicated()
    res = {"out_max_abs_diff": float((o1.float() - o2.float()).abs().max()), "lse_max_abs_diff": float((l1 - l2).abs().max()),
           "shared_bytes": seg.bytes_in_use(), "replicated_bytes": held(kc) + held(vc)}
    assert res["out_max_abs_diff"] < 2e-3 and res["lse_max_abs_diff"] < 1e-3, res

    def many(fn):
        def f():
            for _ in range(a.launches):
                fn()
        return f

    ga, gb = graph_of(many(shared)), graph_of(many(replicated))
    replay_us(ga, 5)
    replay_us(gb, 5)
    ta, tb = [], []
    for _ in range(a.rounds):
        ta.append(replay_us(ga, a.replays) / a.launches)
        tb.append(replay_us(gb, a.replays) / a.launches)
    res["shared_us"], res["replicated_us"] = round(sum(ta) / len(ta), 2), round(sum(tb) / len(tb), 2)
    res["shared_us_rounds"], res["replicated_us_rounds"] = [round(x, 2) for x in ta], [round(x, 2) for x in tb]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--head-dims", default="128,64")
    ap.add_argument("--n-seqs", default="1,2,8,16")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_shared_segment.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {"tool": "bench_shared_segment", "device": torch.cuda.get_device_name(0), "q_heads": HQ, "kv_heads": HKV, "tokens": T}
    for D in (int(x) for x in a.head_dims.split(",")):
        for n in (int(x) for x in a.n_seqs.split(",")):
            res[f"d{D}_n{n}"] = run(D, n, a, dev)
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

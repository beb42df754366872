"""What one call for several query tokens saves: one layer, batch 8, 7936 compressed tokens and a window of 132 rows, for
n_q = 1, 2, 4 and 8 new tokens per sequence, at two geometries: 32 q / 8 kv heads at head_dim 128 over an arena, and the Llama-3.2-1B
geometry (32 q / 8 kv heads at head_dim 64) over the reference-layout arrays.  Two ways to the same attention:
  multi      ONE MustafarAttention.decode_multi call: mustafar_decode_multi_query (append, decode launch, row kernel)
  stepwise   n_q decode_fused calls over the same cache and window, each appending its row: what a caller does today
Each way is a captured graph of --launches repetitions back to back (the window lengths are set back on the host before each repetition:
the graph holds fixed lengths), timed with device events around --replays replays behind warm-up replays, the two alternated A B A B
in one process; the outputs are compared before anything is timed.  Prints ONE JSON line: per geometry and n_q the microseconds per call
of `multi` and per n_q steps of `stepwise` (mean of the rounds, and every round).
--mask pad | tree: both ways carry an additive fp16 mask -- `pad`: one row for all tokens, sequence b left-padded by 17 b
columns; `tree`: a row per token, the binary tree parent(j) = (j - 1) // 2 among the new tokens (a decode_fused step takes row j cut to
its columns) -- and a third graph times the UNMASKED multi call on the same operands, alternated with the other two: `multi_unmasked_us`.
Needs an MI355X; it does not fall back to anything.  Usage: python tools/bench_multi_query.py [--launches 20] [--replays 20] [--rounds 4]
[--mask none|pad|tree]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mustafar_amd.hook import MustafarAttention, MustafarConfig  # noqa: E402

HQ, HKV, BSZ, T, W0, S = 32, 8, 8, 7936, 132, 0.7


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


def run(D, n_q, a, dev):
    attn = MustafarAttention(MustafarConfig(num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D, k_sparsity=S, v_sparsity=S,
                                            api="fused", arena=(D == 128)))
    g = torch.Generator(device=dev).manual_seed(D + n_q)
    L0 = T + W0
    K = torch.randn((BSZ, HKV, L0 + n_q, D), generator=g, device=dev).half()
    V = torch.randn((BSZ, HKV, L0 + n_q, D), generator=g, device=dev).half()
    q = torch.randn((BSZ, HQ, n_q, D), generator=g, device=dev).half()
    k_c, k_w, v_c, v_w, C, _ = attn.to_fused(attn.build_cache(K[:, :, :L0].contiguous(), V[:, :, :L0].contiguous()))
    assert C == T and k_w.len == W0
    kn, vn = K[:, :, L0:].contiguous(), V[:, :, L0:].contiguous()
    qs = [q[:, :, j:j + 1].contiguous() for j in range(n_q)]
    ks = [kn[:, :, j:j + 1].contiguous() for j in range(n_q)]
    vs = [vn[:, :, j:j + 1].contiguous() for j in range(n_q)]
    del K, V
    mask = None
    if a.mask != "none":
        lowest = torch.finfo(torch.float16).min
        mask = torch.zeros((BSZ, 1, 1 if a.mask == "pad" else n_q, L0 + n_q), dtype=torch.float16, device=dev)
        for b in range(BSZ if a.mask == "pad" else 0):
            mask[b, :, :, :17 * b] = lowest
        for j in range(n_q if a.mask == "tree" else 0):
            seen, i = set(), j
            while i >= 0:
                seen.add(i)
                i = (i - 1) // 2 if i else -1
            mask[:, :, j, [L0 + i for i in range(n_q) if i not in seen]] = lowest
    step_masks = [None if mask is None else mask[:, :, min(j, mask.shape[2] - 1):min(j, mask.shape[2] - 1) + 1, :L0 + j + 1] for j in range(n_q)]

    def multi(m=mask):
        k_w.len = v_w.len = W0
        return attn._decode_multi_call(q, kn, vn, (k_c, k_w, v_c, v_w, C, L0), m)[0]

    def stepwise():
        outs = []
        for j in range(n_q):
            k_w.len = v_w.len = W0 + j
            outs.append(attn.decode_fused(qs[j], ks[j], vs[j], (k_c, k_w, v_c, v_w, C, L0 + j), attention_mask=step_masks[j])[0])
        return outs

    o1, o2 = multi(), torch.cat(stepwise(), dim=2)
    res = {"out_max_abs_diff": float((o1.float() - o2.float()).abs().max())}
    assert res["out_max_abs_diff"] < 2e-3, res

    def many(fn):
        def f():
            for _ in range(a.launches):
                fn()
        return f

    ga, gb = graph_of(many(multi)), graph_of(many(stepwise))
    gu = graph_of(many(lambda: multi(None))) if mask is not None else None
    replay_us(ga, 5)
    replay_us(gb, 5)
    ta, tb, tu = [], [], []
    for _ in range(a.rounds):
        ta.append(replay_us(ga, a.replays) / a.launches)
        tb.append(replay_us(gb, a.replays) / a.launches)
        if gu is not None:
            tu.append(replay_us(gu, a.replays) / a.launches)
    res["multi_us"], res["stepwise_us"] = round(sum(ta) / len(ta), 2), round(sum(tb) / len(tb), 2)
    res["multi_us_rounds"], res["stepwise_us_rounds"] = [round(x, 2) for x in ta], [round(x, 2) for x in tb]
    if tu:
        res["multi_unmasked_us"], res["multi_unmasked_us_rounds"] = round(sum(tu) / len(tu), 2), [round(x, 2) for x in tu]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--head-dims", default="128,64")
    ap.add_argument("--n-q", default="1,2,4,8")
    ap.add_argument("--mask", choices=["none", "pad", "tree"], default="none")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_multi_query.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {"tool": "bench_multi_query", "device": torch.cuda.get_device_name(0), "q_heads": HQ, "kv_heads": HKV, "batch": BSZ, "tokens": T,
           "window": W0, "mask": a.mask}
    for D in (int(x) for x in a.head_dims.split(",")):
        for n in (int(x) for x in a.n_q.split(",")):
            res[f"d{D}_nq{n}"] = run(D, n, a, dev)
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

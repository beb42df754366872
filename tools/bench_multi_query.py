"""What one call for several query tokens saves: one layer, batch 8, 7936 compressed tokens and a window of 132 rows, for
n_q = 1, 2, 4 and 8 new tokens per sequence, at two geometries: 32 q / 8 kv heads at head_dim 128 over an arena, and the Llama-3.2-1B
geometry (32 q / 8 kv heads at head_dim 64) over the reference-layout arrays.  Two ways to the same attention:
  multi      ONE MustafarAttention.decode_multi call: mustafar_decode_multi_query (append, decode launch, row kernel)
  stepwise   n_q decode_fused calls over the same cache and window, each appending its row: what a caller does today
--lengths: one call, the fixed-length graph against the device-length graphs of ABI 115 at the same state (run_lengths).
--loop [--layers 32]: a verify loop of 64 rounds of n_q = 4, eager decode_multi + accept against one replayed graph (run_loop; --rounds
alternations, 2 are plenty).
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
import time

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

    if a.lengths:
        return run_lengths(attn, many, multi, (q, kn, vn), (k_c, k_w, v_c, v_w, C, L0), res, a, dev)
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


def time_lengths(attn, many, qkv, past, caps, res, prefix, a, dev):
    """The fixed-length graph of the unmasked call against its device-length graphs at the state `past` (window length past[1].len): the
    counter at 0 (`counter_us`) and, for every capacity in `caps`, the compressed tokens in use on the device as well (`t_device_us` at
    the compressed length itself: the same grid; `t_device_cap<N>_us`: N tokens of capacity more, their runs launched and skipped) --
    alternated, --rounds rounds."""
    k_c, k_w, v_c, v_w, C, L0 = past
    W = k_w.len
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    t_dev = torch.tensor([C], dtype=torch.int32, device=dev)

    def call(*lengths, **kw):
        def f():
            k_w.len = v_w.len = W
            return attn._decode_multi_call(*qkv, (k_c, k_w, v_c, v_w, C, L0), None, *lengths, **kw)[0]
        return f

    legs = {"fixed_us": call(), "counter_us": call(counter)}
    for cap in caps:
        legs["t_device_us" if cap == C else f"t_device_cap{cap - C}_us"] = call(counter, t_device=t_dev, T=cap)
    want = legs["fixed_us"]().clone()
    for name, fn in legs.items():
        assert float((fn().float() - want.float()).abs().max()) < 2e-3, name
    graphs = {name: graph_of(many(fn)) for name, fn in legs.items()}
    times = {name: [] for name in legs}
    for g in graphs.values():
        replay_us(g, 5)
    for _ in range(a.rounds):
        for name, g in graphs.items():
            times[name].append(replay_us(g, a.replays) / a.launches)
    for name, t in times.items():
        res[prefix + name], res[prefix + name + "_rounds"] = round(sum(t) / len(t), 2), [round(x, 2) for x in t]


def run_lengths(attn, many, multi, qkv, past, res, a, dev):
    """--lengths: `time_lengths` at the state of the other legs (an arena that is its base alone launches the plain instantiation for
    the fixed call and the extents one under `t_device`: `t_device_cap256_us` there compares two instantiations), and, for an arena,
    at the same lengths with the last 256 compressed tokens in an EXTENT (`ext_*`): every graph then runs the extents instantiation,
    and `ext_t_device_us` against `ext_fixed_us` is the price of the device-side compressed length, like for like."""
    k_c, k_w, v_c, v_w, C, L0 = past
    arena = hasattr(k_c, "ext_table")
    time_lengths(attn, many, qkv, past, [C + 256] if arena else [], res, "", a, dev)
    if not arena:
        return res
    D, g = qkv[0].shape[3], torch.Generator(device=dev).manual_seed(7)
    n0 = C - 256 + attn.cfg.residual_length + 255           # one step short of the trigger that lists the extent
    K = torch.randn((BSZ, HKV, n0 + 1, D), generator=g, device=dev).half()
    V = torch.randn((BSZ, HKV, n0 + 1, D), generator=g, device=dev).half()
    grown = attn.to_fused(attn.build_cache(K[:, :, :n0].contiguous(), V[:, :, :n0].contiguous()))
    _, grown = attn.decode_fused(qkv[0][:, :, :1].contiguous(), K[:, :, n0:], V[:, :, n0:], grown)
    e_k, e_kw, e_v, e_vw, e_C, _ = grown
    assert e_C == C and e_k.tokens == C - 256 and len(e_k.extents) == 1 and e_kw.len == attn.cfg.residual_length
    e_kw.buf[:, :, e_kw.len:W0] = K[:, :, :W0 - e_kw.len]    # the window of the other legs: W0 rows
    e_vw.buf[:, :, e_vw.len:W0] = V[:, :, :W0 - e_vw.len]
    e_kw.len = e_vw.len = W0
    time_lengths(attn, many, qkv, (e_k, e_kw, e_v, e_vw, C, L0), [C, C + 256], res, "ext_", a, dev)
    return res


REJECTED = [0, 1, 0, 3, 0, 0, 2, 0]   # --loop: drafts rejected per round, cycled


def run_loop(D, a, dev):
    """--loop: a speculative verify loop over --layers layers at the shape of the other legs, n_q = 4, 64 rounds, REJECTED drafts per
    round, wall clock around the whole loop (the host is what is measured), on caches built anew for every leg.
      eager     per round and layer decode_multi + accept(rejected)
      replayed  ONE captured graph of the layers' decode_multi calls with the lengths on the device; per round a replay, per layer
                accept(advance(past, 4), rejected), once the counter; the rounds in front of a trigger point (fits_before_trigger < 4)
                run eagerly, and the trigger runs inside accept in both legs (the window reaches it once: 132 -> 288 rows)
    The cache grows by extents at both head dims (arena at 128, ExtentCache64 at 64), so the one graph serves the whole loop."""
    from mustafar_amd import _lib
    L_ = _lib.load()
    n_q, rounds = 4, 64
    kinds = dict(arena=True) if D == 128 else dict(hd64_extents=True)
    attn = MustafarAttention(MustafarConfig(num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D, k_sparsity=S, v_sparsity=S,
                                            api="fused", **kinds))
    g = torch.Generator(device=dev).manual_seed(D)
    L0 = T + W0
    K = torch.randn((BSZ, HKV, L0, D), generator=g, device=dev).half()
    V = torch.randn((BSZ, HKV, L0, D), generator=g, device=dev).half()
    q = torch.randn((BSZ, HQ, n_q, D), generator=g, device=dev).half()
    kn = torch.randn((BSZ, HKV, n_q, D), generator=g, device=dev).half()
    vn = torch.randn((BSZ, HKV, n_q, D), generator=g, device=dev).half()

    def fresh():
        return [attn.to_fused(attn.build_cache(K, V)) for _ in range(a.layers)]

    def eager_round(pasts, fit, rej):
        for l, p in enumerate(pasts):
            _, p = attn.decode_multi(q[:, :, :fit], kn[:, :, :fit], vn[:, :, :fit], p)
            pasts[l] = attn.accept(p, rejected=rej)

    def loop(replayed):
        pasts = fresh()
        C = pasts[0][4]
        assert C == T and pasts[0][1].len == W0
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        t_dev = torch.tensor([C], dtype=torch.int32, device=dev)
        gq, gk, gv = q.clone(), kn.clone(), vn.clone()
        graph = None
        if replayed:
            graph = graph_of(lambda: [attn.decode_multi(gq, gk, gv, p, step_counter=counter, t_device=t_dev, t_capacity=C + 256)
                                      for p in pasts])
        else:
            eager_round([tuple(p[:1]) + (p[1].clone(), p[2], p[3].clone()) + tuple(p[4:]) for p in pasts], n_q, 0)   # (warm)
        st = torch.cuda.current_stream().cuda_stream
        kept = on_graph = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(rounds):
            fit = attn.fits_before_trigger(pasts[0], n_q)
            rej = min(REJECTED[i % len(REJECTED)], fit - 1)
            before = pasts[0][4]
            if replayed and fit == n_q:
                gq.copy_(q); gk.copy_(kn); gv.copy_(vn)
                graph.replay()
                for l, p in enumerate(pasts):
                    pasts[l] = attn.accept(attn.advance(p, n_q), rejected=rej)
                on_graph += 1
            else:
                eager_round(pasts, fit, rej)
            if replayed:
                L_.mustafar_counter_add(st, counter.data_ptr(), fit - rej)
                if pasts[0][4] != before:
                    t_dev.add_(256)
                    counter.sub_(256)
            kept += fit - rej
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert pasts[0][4] == T + 256 and pasts[0][1].len == W0 + kept - 256
        return {"ms_per_round": round(dt * 1e3 / rounds, 3), "accepted_tokens_per_s": round(BSZ * kept / dt, 1), "graph_rounds": on_graph}

    res = {"layers": a.layers, "rounds": rounds, "n_q": n_q, "eager": [], "replayed": []}
    for _ in range(a.rounds):
        res["eager"].append(loop(False))
        res["replayed"].append(loop(True))
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--head-dims", default="128,64")
    ap.add_argument("--n-q", default="1,2,4,8")
    ap.add_argument("--mask", choices=["none", "pad", "tree"], default="none")
    ap.add_argument("--lengths", action="store_true", help="one call: the fixed-length graph against the device-length graph (ABI 115)")
    ap.add_argument("--loop", action="store_true", help="a speculative verify loop over --layers layers: eager against one replayed graph (ABI 115)")
    ap.add_argument("--layers", type=int, default=32)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_multi_query.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {"tool": "bench_multi_query", "device": torch.cuda.get_device_name(0), "q_heads": HQ, "kv_heads": HKV, "batch": BSZ, "tokens": T,
           "window": W0, "mask": a.mask}
    for D in (int(x) for x in a.head_dims.split(",")):
        if a.loop:
            res[f"d{D}_loop"] = run_loop(D, a, dev)
            continue
        for n in (int(x) for x in a.n_q.split(",")):
            res[f"d{D}_nq{n}"] = run(D, n, a, dev)
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

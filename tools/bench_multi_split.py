"""What one call for several query tokens saves next to a shared prefix: one layer, 32 q / 8 kv heads, batch 8, a shared
prefix of 7936 tokens held ONCE plus, per sequence, a live cache of 256 compressed tokens and a window of 132 rows, 70 % / 70 % sparsity,
head_dim 128 (live cache in an arena) and 64 (reference-layout arrays), n_q = 1, 2, 4 and 8 new tokens per sequence.  Three ways:
  A  split_multi   ONE MustafarAttention.decode_multi_split: mustafar_decode_shared_segment_multi over the prefix, decode_multi over the
                   live cache, one merge
  B  split_steps   n_q decode_split steps over the same prefix and live cache, each appending its row: what a caller did before
  C  multi_whole   ONE decode_multi over the same tokens held once PER SEQUENCE (8 x the prefix bytes): no shared copy, no merge
Each way is a captured graph of --launches repetitions back to back (the window lengths are set back on the host before each repetition:
the graph holds fixed lengths), timed with device events around --replays replays behind warm-up replays, alternated A B C A B C in one
process; the outputs are compared before anything is timed.
`shared_chunks`: the shared call alone (SharedSegment.decode_multi over the prefix) at 1, 2, 4 and 8 chunks of 64 rows per kv head -- batch
8 x GQA-4 x n_q = 2, 4, 8, 16 --, the same way: what one more chunk, i.e. one more expansion of every block, costs.
Prints ONE JSON line.  Needs an MI355X; it does not fall back to anything.
Usage: python tools/bench_multi_split.py [--launches 20] [--replays 20] [--rounds 4] [--head-dims 128,64] [--n-q 1,2,4,8]
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
from mustafar_amd.hook import MustafarAttention, MustafarConfig  # noqa: E402
from tools.bench_multi_query import graph_of, replay_us  # noqa: E402

HQ, HKV, BSZ, F, C_LIVE, W0, S = 32, 8, 8, 7936, 256, 132, 0.7


def alternate(graphs, a):
    """{name: us per repetition, mean of the rounds} and {name: every round} of captured graphs replayed in turn."""
    for g in graphs.values():
        replay_us(g, 5)
    times = {name: [] for name in graphs}
    for _ in range(a.rounds):
        for name, g in graphs.items():
            times[name].append(replay_us(g, a.replays) / a.launches)
    res = {}
    for name, t in times.items():
        res[name + "_us"], res[name + "_us_rounds"] = round(sum(t) / len(t), 2), [round(x, 2) for x in t]
    return res


def many(fn, a):
    def f():
        for _ in range(a.launches):
            fn()
    return f


def hook(D):
    return MustafarAttention(MustafarConfig(num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D, k_sparsity=S, v_sparsity=S,
                                            api="fused", arena=(D == 128)))


def data(D, n_q, dev):
    g = torch.Generator(device=dev).manual_seed(D + n_q)
    L0 = F + C_LIVE + W0
    K = torch.randn((BSZ, HKV, L0 + n_q, D), generator=g, device=dev).half()
    V = torch.randn((BSZ, HKV, L0 + n_q, D), generator=g, device=dev).half()
    K[1:, :, :F], V[1:, :, :F] = K[:1, :, :F], V[:1, :, :F]          # one prefix
    q = torch.randn((BSZ, HQ, n_q, D), generator=g, device=dev).half()
    return K, V, q, L0


def run(D, n_q, a, dev):
    attn = hook(D)
    K, V, q, L0 = data(D, n_q, dev)
    live = L0 - F
    seg = partial.SharedSegment.from_dense(attn, K[:1, :, :F].contiguous(), V[:1, :, :F].contiguous())
    new_past = lambda lo: attn.to_fused(attn.build_cache(K[:, :, lo:L0].contiguous(), V[:, :, lo:L0].contiguous()))
    pa, pb, pc = new_past(F), new_past(F), new_past(0)
    assert pa[4] == pb[4] == C_LIVE and pc[4] == F + C_LIVE and pa[1].len == pc[1].len == W0
    kn, vn = K[:, :, L0:].contiguous(), V[:, :, L0:].contiguous()
    qs = [q[:, :, j:j + 1].contiguous() for j in range(n_q)]
    ks = [kn[:, :, j:j + 1].contiguous() for j in range(n_q)]
    vs = [vn[:, :, j:j + 1].contiguous() for j in range(n_q)]
    del K, V

    def at(p, w, L):
        p[1].len = p[3].len = w
        return p._replace(kv_seq_len=L)

    def split_multi():
        return attn.decode_multi_split(q, kn, vn, at(pa, W0, live), [seg])[0]

    def split_steps():
        return [attn.decode_split(qs[j], ks[j], vs[j], at(pb, W0 + j, live + j), [seg])[0] for j in range(n_q)]

    def multi_whole():
        return attn.decode_multi(q, kn, vn, at(pc, W0, L0))[0]

    oa, ob, oc = split_multi(), torch.cat(split_steps(), dim=2), multi_whole()
    res = {"split_multi_vs_steps_max_abs_diff": float((oa.float() - ob.float()).abs().max()),
           "split_multi_vs_whole_max_abs_diff": float((oa.float() - oc.float()).abs().max())}
    assert max(res.values()) < 2e-3, res
    res.update(alternate({"split_multi": graph_of(many(split_multi, a)), "split_steps": graph_of(many(split_steps, a)),
                          "multi_whole": graph_of(many(multi_whole, a))}, a))
    return res


def run_chunks(D, a, dev):
    attn = hook(D)
    g = torch.Generator(device=dev).manual_seed(D)
    K = torch.randn((1, HKV, F, D), generator=g, device=dev).half()
    V = torch.randn((1, HKV, F, D), generator=g, device=dev).half()
    seg = partial.SharedSegment.from_dense(attn, K, V)
    groups, graphs = HQ // HKV, {}
    for chunks in (1, 2, 4, 8):
        n_q = chunks * 64 // (BSZ * groups)
        q = torch.randn((BSZ, HQ, n_q, D), generator=g, device=dev).half()
        graphs[f"chunks{chunks}_nq{n_q}"] = graph_of(many(lambda q=q: seg.decode_multi(attn, q), a))
    return alternate(graphs, a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--head-dims", default="128,64")
    ap.add_argument("--n-q", default="1,2,4,8")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_multi_split.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {"tool": "bench_multi_split", "device": torch.cuda.get_device_name(0), "q_heads": HQ, "kv_heads": HKV, "batch": BSZ,
           "shared_tokens": F, "live_tokens": C_LIVE, "window": W0}
    for D in (int(x) for x in a.head_dims.split(",")):
        for n in (int(x) for x in a.n_q.split(",")):
            res[f"d{D}_nq{n}"] = run(D, n, a, dev)
            torch.cuda.empty_cache()
        res[f"d{D}_shared_chunks"] = run_chunks(D, a, dev)
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

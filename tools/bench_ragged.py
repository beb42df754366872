"""What the ragged call costs next to what a caller does today: one layer, batch 8, 32 q / 8 kv heads at head_dim 128
(Llama-3-8B; caches in arenas) and at head_dim 64 (Llama-3.2-1B; reference-layout arrays), 70 % / 70 % sparsity, n_q = 1 and 4 new tokens
per sequence.  The sequences hold 512, 1024, 2048, 2048, 4096, 4096, 8192 and 8192 compressed tokens and a window of 132 rows each.
Three ways:
  a  ragged     ONE MustafarAttention.decode_ragged over eight bsz-1 pasts (mustafar_ragged_set_sequences + mustafar_decode_ragged)
  b  padded     ONE decode_multi over the rectangle left-padded to the longest sequence, with the mask that hides the padding: the pad
                tokens are compressed, stored and read like any others
  c  per_seq    eight bsz-1 decode_multi calls
and two more batches the same three ways: eight EQUAL sequences of 4096 tokens (`_equal`), where `b` is decode_multi over the rectangle
itself, without a mask -- what `a` should cost there --, and seven sequences of 512 tokens next to one of 8192 (`_skewed`): the grid is
sized for 8192 tokens and 87 % of its compressed-run workgroups find nothing of their sequence to serve, so it shows whether `a` follows
the sum of the lengths or the grid.  Each way is a captured graph of --launches repetitions back to back (the host lengths are set back
before each repetition: a call appends its rows), timed with device events around --replays replays behind warm-up replays, alternated
a b c a b c for --rounds rounds in one process.  The outputs are compared before anything is timed: a == c bit for bit, a against b
within 2e-3.  `*_bytes`: what a call has to read, from the objects -- the compressed bytes in use plus the window rows -- not a counter.
Prints ONE JSON line.  Needs an MI355X; it does not fall back to anything.
Usage: python tools/bench_ragged.py [--launches 10] [--replays 20] [--rounds 5] [--head-dims 128,64] [--n-q 1,4]
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
from mustafar_amd.reflayout import as_cache  # noqa: E402
from tools.bench_multi_query import graph_of, replay_us  # noqa: E402

HQ, HKV, S, W0 = 32, 8, 0.7, 132
LENGTHS = (512, 1024, 2048, 2048, 4096, 4096, 8192, 8192)
EQUAL = (4096,) * 8
SKEWED = (512,) * 7 + (8192,)
NEG = torch.finfo(torch.float16).min


def hook(D):
    return MustafarAttention(MustafarConfig(num_attention_heads=HQ, num_key_value_heads=HKV, head_dim=D, k_sparsity=S, v_sparsity=S,
                                            api="fused", arena=(D == 128)))


def past_bytes(past, n_q):
    """Bytes a call over `past` has to read: both compressed caches as they are held, and the window rows in use behind the append."""
    k_c, k_w, v_c, v_w, C, _ = past
    win = 2 * k_w.buf.shape[0] * k_w.buf.shape[1] * (k_w.len + n_q) * k_w.buf.shape[3] * 2
    return (as_cache(k_c, C).bytes_in_use() + as_cache(v_c, C).bytes_in_use() if C else 0) + win


def alternate(graphs, a):
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


def run(D, n_q, lengths, a, dev, masked):
    """The three ways over sequences of `lengths` compressed tokens (+ W0 window rows).  masked: the rectangle needs the padding mask."""
    attn = hook(D)
    n, Lmax = len(lengths), max(lengths) + W0
    g = torch.Generator(device=dev).manual_seed(D + n_q + len(set(lengths)))
    K = torch.zeros((n, HKV, Lmax + n_q, D), dtype=torch.float16, device=dev)   # left-padded: sequence s in columns [Lmax - L_s, Lmax + n_q)
    V = torch.zeros_like(K)
    mask = torch.zeros((n, 1, 1, Lmax + n_q), dtype=torch.float16, device=dev)
    for s, T in enumerate(lengths):
        pad = Lmax - (T + W0)
        K[s, :, pad:] = torch.randn((HKV, T + W0 + n_q, D), generator=g, device=dev).half()
        V[s, :, pad:] = torch.randn((HKV, T + W0 + n_q, D), generator=g, device=dev).half()
        mask[s, :, :, :pad] = NEG
    q = torch.randn((n, HQ, n_q, D), generator=g, device=dev).half()
    kn, vn = K[:, :, Lmax:].contiguous(), V[:, :, Lmax:].contiguous()
    seq_past = lambda s: attn.to_fused(attn.build_cache(K[s:s + 1, :, Lmax - lengths[s] - W0:Lmax].contiguous(),
                                                        V[s:s + 1, :, Lmax - lengths[s] - W0:Lmax].contiguous()))
    pa, pc = [seq_past(s) for s in range(n)], [seq_past(s) for s in range(n)]
    pb = attn.to_fused(attn.build_cache(K[:, :, :Lmax].contiguous(), V[:, :, :Lmax].contiguous()))
    assert [p[4] for p in pa] == list(lengths) and pb[4] == max(lengths) and all(p[1].len == W0 for p in pa + [pb])
    del K, V
    qs, ks, vs = ([t[s:s + 1].contiguous() for s in range(n)] for t in (q, kn, vn))

    def at(p, L):
        p[1].len = p[3].len = W0
        return p._replace(kv_seq_len=L)

    def ragged():
        return attn.decode_ragged(q, kn, vn, [at(p, T + W0) for p, T in zip(pa, lengths)])[0]

    def rect():
        return attn.decode_multi(q, kn, vn, at(pb, Lmax), attention_mask=mask if masked else None)[0]

    def per_seq():
        return torch.cat([attn.decode_multi(qs[s], ks[s], vs[s], at(pc[s], lengths[s] + W0))[0] for s in range(n)])

    oa, ob, oc = ragged(), rect(), per_seq()
    res = {"ragged_vs_per_seq_bit_equal": bool(torch.equal(oa.view(torch.int16), oc.view(torch.int16))),
           "ragged_vs_rect_max_abs_diff": float((oa.float() - ob.float()).abs().max())}
    assert res["ragged_vs_per_seq_bit_equal"] and res["ragged_vs_rect_max_abs_diff"] < 2e-3, res
    res["ragged_bytes"] = res["per_seq_bytes"] = sum(past_bytes(at(p, 0), n_q) for p in pa)
    res["rect_bytes"] = past_bytes(at(pb, 0), n_q)
    res["compressed_tokens"] = sum(lengths)
    res["rect_compressed_tokens"] = n * max(lengths)

    def many(fn):
        def f():
            for _ in range(a.launches):
                fn()
        return f

    res.update(alternate({"ragged": graph_of(many(ragged)), "rect": graph_of(many(rect)), "per_seq": graph_of(many(per_seq))}, a))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--head-dims", default="128,64")
    ap.add_argument("--n-q", default="1,4")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/bench_ragged.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {"tool": "bench_ragged", "device": torch.cuda.get_device_name(0), "q_heads": HQ, "kv_heads": HKV, "batch": len(LENGTHS),
           "lengths": list(LENGTHS), "equal": list(EQUAL), "skewed": list(SKEWED), "window": W0, "launches": a.launches, "replays": a.replays, "rounds": a.rounds}
    for D in (int(x) for x in a.head_dims.split(",")):
        for n_q in (int(x) for x in a.n_q.split(",")):
            res[f"d{D}_nq{n_q}"] = run(D, n_q, LENGTHS, a, dev, masked=True)      # rect = the padded rectangle behind its mask
            torch.cuda.empty_cache()
            res[f"d{D}_nq{n_q}_equal"] = run(D, n_q, EQUAL, a, dev, masked=False)   # rect = the rectangle itself, no mask
            torch.cuda.empty_cache()
            res[f"d{D}_nq{n_q}_skewed"] = run(D, n_q, SKEWED, a, dev, masked=True)
            torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

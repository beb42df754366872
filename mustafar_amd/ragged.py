"""Ragged batches: n bsz-1 pasts of one MustafarAttention decoded in ONE call (mustafar_ragged_set_sequences + mustafar_decode_ragged;
ragged_batch.hip).

A server's sequences have prompts of different lengths, join and leave at different steps and accept different numbers of drafted
tokens.  `decode_multi` takes a rectangle: it serves such a batch left-padded to the longest sequence behind a mask -- the pad tokens
are pruned, compressed, stored and read on every step -- or as one bsz-1 call per sequence.  Here each sequence keeps a bsz-1 `past`
of its own, so the trigger, `accept(rejected=)`, `accept(keep=)`, arenas, extents and ExtentCache64 work per sequence unchanged; a
batch is whatever list of pasts the caller hands over at this step, and one launch reads only the tokens that exist.

    batch = RaggedBatch(attn, capacity=64)                     # owns the device table; create it outside any graph capture
    out, pasts = batch.decode(q, k, v, pasts)                  # q [n, H, n_q, D], k / v [n, Hkv, n_q, D], n <= capacity pasts
    pasts = [attn.accept(p, rejected=r) for p, r in zip(pasts, rejected)]   # per sequence: its own drafts, its own trigger

This module imports nothing from hook.py (hook.py imports it): an attention object is asked for `to_fused`, `fits_before_trigger`,
`_multi_shapes` and `_scratch`, a past is the tuple `to_fused` returns.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from .reflayout import as_cache

SEQUENCE_BYTES = ctypes.sizeof(_lib.Sequence)   # 176


def _window_shape(w):
    """(bsz, rows in use, the tensor) of a window: a `hook.Window` (api="fused") or the dense tensor of a reference-layout past."""
    if hasattr(w, "buf"):
        return w.buf.shape[0], w.len, w.buf
    return w.shape[0], w.shape[2], w


class RaggedBatch:
    """The device table of `capacity` sequences and the call over it.  One object serves any number of calls; the table is created
    at the first call on the query's device, which must not be under graph capture."""

    def __init__(self, attn, capacity: int):
        if attn.cfg.api != "fused":
            raise ValueError("RaggedBatch needs MustafarConfig(api='fused')")
        if not isinstance(capacity, int) or not 1 <= capacity <= 65535 // attn.num_key_value_heads:
            raise ValueError(f"RaggedBatch: capacity must be in [1, {65535 // attn.num_key_value_heads}] sequences of "
                             f"{attn.num_key_value_heads} kv heads (got {capacity!r})")
        self.attn, self.capacity = attn, capacity
        self.table = None

    def _table(self, dev) -> torch.Tensor:
        if self.table is None or self.table.device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RaggedBatch: the device table must exist before a graph is captured (issue one call outside the capture)")
            self.table = torch.zeros(self.capacity * SEQUENCE_BYTES, dtype=torch.uint8, device=dev)   # all zero: every slot empty
        return self.table

    def _check(self, query_states, key_states, value_states, pasts) -> int:
        """Everything a call refuses, before any device work and before any past is touched -> n_q."""
        attn = self.attn
        n_q = attn._multi_shapes("decode_ragged", query_states, key_states, value_states)
        n, groups = query_states.shape[0], attn.num_key_value_groups
        if len(pasts) != n:
            raise ValueError(f"decode_ragged: one bsz-1 past per sequence of the query (got {len(pasts)} pasts for {n} sequences)")
        if not 1 <= n <= self.capacity:
            raise ValueError(f"decode_ragged: 1 to {self.capacity} sequences, the capacity of this RaggedBatch (got {n})")
        if n_q > 64 // groups:
            raise ValueError(f"decode_ragged is one library call: at most {64 // groups} tokens at {groups} q heads per kv head "
                             f"(got {n_q}); split the tokens over consecutive calls")
        for s, past in enumerate(pasts):
            if len(past) != 6:
                raise ValueError(f"decode_ragged: sequence {s} is not a past (the 6-tuple of build_cache / to_fused)")
            for w in (past[1], past[3]):
                if _window_shape(w)[0] != 1:
                    raise ValueError(f"decode_ragged: sequence {s} is not a bsz-1 past (its windows hold {_window_shape(w)[0]} sequences)")
            fits = attn.fits_before_trigger(past, n_q)
            if fits < n_q:
                raise ValueError(f"decode_ragged: sequence {s}: {n_q} tokens would step over its 256-token trigger point; at most {fits} fit "
                                 "in this call (the trigger point may only be the last row: accept() then runs the trigger)")
        return n_q

    def decode(self, query_states, key_states, value_states, pasts, return_lse: bool = False):
        """n_q consecutive tokens of each of n sequences: q [n, H, n_q, D], their new k / v [n, Hkv, n_q, D], `pasts` a list of n bsz-1
        pasts of this attention object -> (out [n, H, n_q, D], pasts'), or (out, lse fp32 [n, H, n_q], pasts') with `return_lse`.  Token
        j of sequence s attends to its own cache, its own window and its own new rows 0 .. j: bit for bit what
        `decode_multi(q[s:s+1], ...)` on that past alone returns.  The call appends the rows and never compresses: close it per sequence
        with `accept()`.  ValueError before anything is touched for: api != "fused", shapes, len(pasts) != n, n beyond the capacity,
        n_q > 64 // groups, a past that is not bsz 1, a sequence that would step over its trigger point (naming it and the n_q that fits).

        Every cache kind decode_multi serves works, mixed freely: a reference-layout list, nothing compressed yet, a CompressedArena with
        extents or in place, an ExtentCache64.  The entries are built from `as_cache(...).view_args(...)`: on an arena that call retiles
        a base held in a base form (key rows, value lists) back to tiles, exactly as decode_multi does -- a bsz-1 `to_fused` normally
        leaves tiles, because `_retile_where_read` asks the launch-shape rule."""
        attn = self.attn
        n_q = self._check(query_states, key_states, value_states, pasts)
        n, H, _, D = query_states.shape
        Hkv, groups, dev = attn.num_key_value_heads, attn.num_key_value_groups, query_states.device
        pasts = [attn.to_fused(p) for p in pasts]
        table = self._table(dev)
        items = (_lib.Sequence * n)()
        keeps, T_max, cap_max = [], 0, n_q
        for it, past in zip(items, pasts):
            k_c, k_w, v_c, v_w, C = past[:5]
            k_w.reserve(k_w.len + n_q)
            v_w.reserve(v_w.len + n_q)
            if k_w.cap != v_w.cap or k_w.len != v_w.len:
                raise RuntimeError("key/value windows must have the same length and capacity")
            k = as_cache(k_c, C)   # (an arena is poll()ed by view_args and a base in a base form retiled; an ExtentCache64 names its tables)
            (kv, vv, t_base, kt, vt), keep = k.view_args(as_cache(v_c, C), tables=C > k.tokens or k.lse_reads_tables)
            keeps.append(keep)
            if kv is not None:
                it.k_base, it.v_base = kv._obj, vv._obj
            it.k_extents, it.v_extents = kt, vt
            it.k_window, it.v_window = k_w.buf.data_ptr(), v_w.buf.data_ptr()
            it.T_base, it.T, it.window_len, it.window_capacity = t_base, C, k_w.len + n_q, k_w.cap
            T_max, cap_max = max(T_max, C), max(cap_max, k_w.cap)
        L = _lib.load()
        ws_bytes = L.mustafar_decode_ragged_workspace_bytes(T_max, cap_max, n, Hkv, groups, n_q, D)
        if ws_bytes <= 0:
            raise ValueError(f"decode_ragged: the library serves no call of {n} sequences x {n_q} tokens x {groups} q heads per kv head, "
                             f"{T_max} compressed tokens, windows of {cap_max} rows, head_dim {D}")
        _, ws = attn._scratch(dev, 0, 0, ws_bytes)
        q = query_states.contiguous()
        kn, vn = key_states.contiguous(), value_states.contiguous()
        out = torch.empty((n, H, n_q, D), dtype=torch.float16, device=dev)
        lse = torch.empty((n, H, n_q), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(L.mustafar_ragged_set_sequences(st, table.data_ptr(), 0, n, items, Hkv, n_q, D), "mustafar_ragged_set_sequences")
            _lib.check(L.mustafar_decode_ragged(st, table.data_ptr(), n, Hkv, groups, n_q, T_max, cap_max, q.data_ptr(), kn.data_ptr(),
                                                vn.data_ptr(), out.data_ptr(), lse.data_ptr(), ws.data_ptr(), math.sqrt(D), D),
                       "mustafar_decode_ragged")
        del keeps, q, kn, vn   # (alive until here: the calls have been issued)
        new = []
        for past in pasts:
            past[1].len = past[3].len = past[1].len + n_q
            new.append(past._replace(kv_seq_len=past.kv_seq_len + n_q))
        return (out, lse, new) if return_lse else (out, new)

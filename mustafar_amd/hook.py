"""Host-side mirror of the attention hook in models/llama_mustafar_kernel.py (LlamaFlashAttention_MUSTAFAR).

The reference file targets transformers 4.43 + flash-attn and cannot be imported here; what this module
reproduces is the part of `forward` (:199-457) that sits between RoPE and o_proj -- the only part that touches
the Mustafar operators -- with the same cache tuple, the same trigger rule and the same call sequence:

    prefill (:405-445)  dense causal attention, T = ((L - R)//256)*256, prune+compress [:T], window = the rest
    decode  (:256-400)  window append, key SpMV, dense window scores, /sqrt(d), fp32 softmax, value SpMV,
                        dense window p.V, and every 256th step prune+compress the oldest 256 window tokens

`past` is the reference's 6-tuple (k_compressed, k_local_window, v_compressed, v_local_window,
compressed_length, kv_seq_len) (:445), k_compressed = [bitmaps, idxs, nzs(list per kv-head), nz_offset]; `Past` names its fields.
The layers below: reflayout.py (the list's primitives and the protocol by which a cache of any kind arrives at a call), compression.py,
cache.py / cache64.py; their names that callers import from here are re-exported.  partial.py is the one layer above.

`api="reference"` issues exactly the reference's calls (query/probabilities zero-padded to 8 rows :273/:313,
`torch.cat` of the per-head streams on every call :274/:314, 8-row outputs sliced to row 0 :275/:315).
`api="native"` calls the same two entry points un-padded (N = 1) and keeps the packed stream of all heads in
one flat tensor beside the list, so nothing is re-copied per step.
`api="fused"` replaces the PyTorch glue between the two SpMVs by the fused decode call of the C ABI (`_call_decode`):
the local window lives in a preallocated buffer that is appended in place, and one call per layer launches
key SpMV (+ window scores) -> softmax -> value SpMV (+ window p.V partials) -> sum.  All three produce the same output.
"""
from __future__ import annotations

import glob
import importlib.util
import math
import os
from dataclasses import dataclass
from typing import Any, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib, compression, mustafar_package
from .cache import KEY_NIBBLE_ROWS, KEY_ROWS, VALUE_LISTS, VALUE_PAIR_LISTS, BaseForm, CompressedArena
from .cache64 import ExtentCache64, compress_raw_pair_hd64
from .ragged import RaggedBatch
from .compression import _compress                                                                          # noqa: F401  (re-exported)
from .reflayout import FlatStreams, _flat_stream, append_compressed, as_cache, nz_offset_from_idxs         # noqa: F401  (re-exported)


def _operator_module():
    """The module behind `mustafar_package.mustafar_{key,value}_formulation` in the unfused call sequences: the compiled PyTorch
    extension of the reference's name (mustafar_amd/dropin, built by setup.py on the C ABI: what the reference hook imports,
    ~5 us of host time per call) when it has been built, else the ctypes mirror (~12 us).  Same checks, same C-ABI calls."""
    global _OPERATORS
    if _OPERATORS is None:
        _OPERATORS = mustafar_package
        hits = glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin", "mustafar_package*.so"))
        if hits and os.environ.get("MUSTAFAR_OPERATORS", "compiled") != "ctypes":
            try:
                _lib.load()   # (libmustafar_hip.so first: the extension links against it)
                spec = importlib.util.spec_from_file_location("mustafar_package", hits[0])
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                _OPERATORS = mod
            except Exception:   # an extension built for another torch: the ctypes mirror does the same calls
                _OPERATORS = mustafar_package
    return _OPERATORS


_OPERATORS = None


@dataclass
class MustafarConfig:
    num_attention_heads: int = 32
    num_key_value_heads: int = 8
    head_dim: int = 128
    k_sparsity: float = 0.7
    v_sparsity: float = 0.7
    residual_length: int = 32     # mem_spd_test.py:9, :22
    group_size: int = 32          # carried by the reference config, unused on the kernel path
    api: str = "native"           # "reference" | "native" | "fused"
    arena: bool = False           # api="fused": keep the compressed cache in CompressedArena objects (in-place append)
    extents: bool = True          # arena: a 256-token trigger adds an extent instead of re-housing the cache (cache.py), where the
                                  # decode launch can read extents (GQA groups % 4 == 0, one-pass pair form)
    arena_slack: float = 0.03       # an arena that appends IN PLACE is housed at (1 + arena_slack) x the rows / stream bytes it holds
                                    # (cache.py: DEFAULT_SLACK); one that grows by extents is housed exactly
    # api="fused": this instance's FMA engine ("dot2" | "valu" | "mfma"; None = the process default) and launch structure
    # ("one_pass" | "two_launch"; None = by size).  Carried in every call's `flags` (include/mustafar_hip.h): two instances in
    # one process run what each of them asks for.
    engine: Optional[str] = None
    structure: Optional[str] = None
    # arena, head_dim 128, GQA groups % 4 == 0, engine "valu" or "dot2": to_fused() retiles the key BASE of an arena into token rows
    # (cache.CompressedArena.to_key_rows) where the launch of the call shape reads them (mustafar_decode_reads_key_rows: the one-pass
    # super-block form).  Whatever needs tiles retiles back (CompressedArena.require_tiles).  MUSTAFAR_KEY_ROWS=0 turns it off everywhere
    key_rows: bool = True
    # The token rows with 4-bit channel steps (cache.CompressedArena.to_key_nibble_rows): what to_fused() prefers for the key base next to a
    # value base that took the lists over pairs of blocks.  None: from NIBBLE_ROWS_FROM compressed tokens per head on (the form saves
    # bytes, and was measured where the bytes are the time: DESIGN.md 5; a small cache keeps the channel bytes); True: wherever the launch
    # reads it.  False / MUSTAFAR_KEY_NIBBLE_ROWS=0 falls back to the rows with channel bytes; key_rows=False / MUSTAFAR_KEY_ROWS=0 turns
    # both off
    key_nibble_rows: Optional[bool] = None
    # The value base as sorted channel lists (cache.CompressedArena.to_value_lists), in the same launches and by the same rules
    # (mustafar_decode_reads_value_lists).  MUSTAFAR_VALUE_LISTS=0 turns it off everywhere
    value_lists: bool = True
    # The lists over PAIRS of 64-token blocks (cache.CompressedArena.to_value_pair_lists): what to_fused() prefers for the value base.
    # False / MUSTAFAR_VALUE_PAIR_LISTS=0 falls back to the lists per block; value_lists=False / MUSTAFAR_VALUE_LISTS=0 turns both off
    value_pair_lists: bool = True
    # head_dim 64, api="fused", arena=False only: the compressed cache grows by 256-token extents (cache64.py) instead of being
    # re-copied by every trigger, and one captured graph of the step with a device-side T serves every cache length up to its capacity
    hd64_extents: bool = False
    # head_dim 64, api="fused", arena=False only: the prefill is compressed from the raw K / V rows in 256-token chunks and gathered into
    # the reference-layout arrays (cache64.compress_raw_pair_hd64: one read of the rows, one host wait) instead of prune + two
    # conversions.  The same tensors, bit for bit; off by default
    hd64_raw_prefill: bool = False


def repeat_kv(hidden_states: torch.Tensor, n_rep: int) -> torch.Tensor:
    """transformers' repeat_kv as used at model :278, :316."""
    batch, num_key_value_heads, slen, head_dim = hidden_states.shape
    if n_rep == 1:
        return hidden_states
    hidden_states = hidden_states[:, :, None, :, :].expand(batch, num_key_value_heads, n_rep, slen, head_dim)
    return hidden_states.reshape(batch, num_key_value_heads * n_rep, slen, head_dim)


def mask_args(attention_mask: Optional[torch.Tensor], bsz: int, columns: int, dev, row_len: Optional[int] = None, exact: bool = False):
    """The additive fp16 mask of a fused call, checked: `(mask, row stride)` with `mask` the tensor whose address the call takes (the
    caller holds it until the call is issued), or `(None, 0)`.  The mask is [bsz, 1, 1, >= columns], `columns` being what the kernels
    read; a column slice of a wider mask keeps its rows the full row apart (rows need no alignment).  `row_len`: the row length the
    error names (the hook's kv_seq_len; default `columns`), which the rows must have exactly when `exact` -- an eager step.  A replayed
    graph reads more columns as its window grows, so there only the lower bound holds."""
    if attention_mask is None:
        return None, 0
    if row_len is None:
        row_len = columns
    if attention_mask.dim() != 4 or attention_mask.shape[:3] != (bsz, 1, 1) or attention_mask.shape[3] < columns or \
            (exact and attention_mask.shape[3] != row_len):
        raise ValueError(f"Attention mask should be of size {(bsz, 1, 1, row_len)}, but is {tuple(attention_mask.size())}")   # :294-297
    if attention_mask.dtype != torch.float16 or attention_mask.device != dev:
        raise RuntimeError("attention_mask must be a float16 tensor on the device of the query")
    if attention_mask.stride(3) != 1:
        attention_mask = attention_mask.contiguous()
    return attention_mask, (attention_mask.stride(0) if bsz > 1 else attention_mask.shape[3])


class Past(NamedTuple):
    """The reference's cache tuple (model :445) with names.  Still a tuple: it compares equal to the plain 6-tuple, unpacks, and indexes
    by `[4]` and `[-1]`; every public method takes either and hands back a `Past`."""
    k_cache: Any             # [bitmaps, idxs, nzs, nz_offset] | CompressedArena | ExtentCache64 | None (nothing compressed yet)
    k_window: Any            # dense tensor [B, Hkv, w, D], or a `Window` (api="fused")
    v_cache: Any
    v_window: Any
    compressed_length: int
    kv_seq_len: int


def _ld_scores(columns: int) -> int:
    """Row pitch of the score scratch for `columns` = compressed tokens + window capacity: rows on 64-byte lines of their own
    (one-pass form: mustafar_hip.h)."""
    return (columns + 31) // 32 * 32


class DecodeOperands(NamedTuple):
    """What `MustafarAttention._decode_operands` builds for one fused call."""
    out: torch.Tensor    # [bsz, num_heads, 1, D] fp16, written by the call
    tail: tuple          # the arguments every entry point takes behind its cache arguments (`_lib._DECODE_TAIL`: q ... flags)
    keep: tuple          # the tensors whose addresses `tail` carries, alive until the call is issued
    ld: int              # `ld_scores` as in `tail`
    flags: int           # `flags` as in `tail`


def _call_decode(k_c, v_c, T: int, ops: DecodeOperands, D: int, t_device: Optional[torch.Tensor] = None,
                 lse: Optional[torch.Tensor] = None) -> None:
    """Issue ONE fused decode call: the only place that chooses among the seven entry points of the C ABI.  k_c / v_c: the two caches
    (None: nothing compressed yet); T: the compressed tokens the launch is sized for (what `ops` was built with); t_device: the
    tokens in use as a device int, or None; lse: the fp32 tensor the row kernel fills, or None.  Each cache kind says how it
    arrives (`decode_args`: reflayout.ListCache for a list or None, CompressedArena, ExtentCache64): eight arrays, or base views +
    T_base + device tables.  The tables are asked for when the launch reads beyond the base tokens; a kind whose `lse_reads_tables`
    is set (ExtentCache64) also whenever there is an LSE.

        cache                            no LSE                                              LSE
        list / None                      mustafar_decode_attention (D 128) / _hd (D 64)      _lse_hd
        CompressedArena, T == its base   _view                                               _extents_lse_hd, null tables
        CompressedArena, T > its base    _extents (tables, t_device)                         _extents_lse_hd (tables, t_device)
        ExtentCache64, base alone        _hd over the eight arrays of the two bases          _extents_lse_hd (tables, t_device)
        ExtentCache64, extents/t_device  _extents_hd (tables, t_device)                      _extents_lse_hd (tables, t_device)

    Whether the launch form asked for can read a grown arena at all is the caller's business (`_decode_fused`)."""
    L = _lib.load()
    k, v = as_cache(k_c, T), as_cache(v_c, T)
    # (with an LSE and T == T_base the extents form reads the base alone, as the plain launch does)
    cache, keep = k.decode_args(v, tables=T > k.tokens or (lse is not None and k.lse_reads_tables))
    arrays = len(cache) == 8
    td = t_device.data_ptr() if t_device is not None else None
    dev = ops.out.device
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        if arrays and lse is not None:
            err = L.mustafar_decode_attention_lse_hd(st, *cache, *ops.tail, D, lse.data_ptr())
        elif arrays and D == 64:
            err = L.mustafar_decode_attention_hd(st, *cache, *ops.tail, D)
        elif arrays:
            err = L.mustafar_decode_attention(st, *cache, *ops.tail)
        elif lse is not None:
            err = L.mustafar_decode_attention_extents_lse_hd(st, *cache, *ops.tail, td, D, lse.data_ptr())
        elif D == 64:
            err = L.mustafar_decode_attention_extents_hd(st, *cache, *ops.tail, td, D)
        elif cache[3] is None:   # an arena that is its base alone: the two views
            err = L.mustafar_decode_attention_view(st, cache[0], cache[1], *ops.tail)
        else:
            err = L.mustafar_decode_attention_extents(st, *cache, *ops.tail, td)
    _lib.check(err, "mustafar_decode_attention")
    del keep   # (alive until here: the call has been issued)


def merge_states(outs: Sequence[torch.Tensor], lses: Sequence[torch.Tensor]):
    """Merge partial attention states over disjoint token sets: outs[i] fp16 [bsz, H, 1, D] (normalised), lses[i] fp32 [bsz, H].
    Returns (out fp16 [bsz, H, 1, D], lse fp32 [bsz, H]) of the attention over all of them; one launch behind the stacking."""
    n = len(outs)
    if n < 1 or n > 64 or len(lses) != n:
        raise ValueError(f"merge_states: 1 to 64 parts with one LSE each (got {n} outputs, {len(lses)} LSEs)")
    bsz, H, _, D = outs[0].shape
    if D not in (64, 128):
        raise ValueError(f"merge_states: head_dim 64 or 128 (got {D})")
    for o, l in zip(outs, lses):
        if o.shape != outs[0].shape or o.dtype != torch.float16 or tuple(l.shape) != (bsz, H) or l.dtype != torch.float32:
            raise ValueError("merge_states: parts are fp16 [bsz, H, 1, D] outputs with fp32 [bsz, H] LSEs of one shape")
    dev = outs[0].device
    o_all = torch.stack([o.reshape(bsz * H, D) for o in outs])       # [n, BH, D]
    l_all = torch.stack([l.reshape(bsz * H) for l in lses])          # [n, BH]
    out = torch.empty((bsz, H, 1, D), dtype=torch.float16, device=dev)
    lse = torch.empty((bsz, H), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        err = _lib.load().mustafar_merge_attention_states(torch.cuda.current_stream(dev).cuda_stream, o_all.data_ptr(), bsz * H * D,
                                                          l_all.data_ptr(), bsz * H, n, bsz * H, D, out.data_ptr(), lse.data_ptr())
    _lib.check(err, "mustafar_merge_attention_states")
    return out, lse


class Window:
    """Dense local window with spare capacity: `buf` [B, Hkv, cap, D], the first `len` rows are valid (api="fused")."""

    def __init__(self, tensor: torch.Tensor, cap: int):
        B, H, w, D = tensor.shape
        self.buf = torch.empty((B, H, max(cap, w), D), dtype=tensor.dtype, device=tensor.device)
        self.buf[:, :, :w] = tensor
        self.len = w

    @property
    def cap(self) -> int:
        return self.buf.shape[2]

    def view(self) -> torch.Tensor:
        return self.buf[:, :, :self.len]

    def reserve(self, n: int):
        if n > self.cap:
            nb = torch.empty((self.buf.shape[0], self.buf.shape[1], n, self.buf.shape[3]), dtype=self.buf.dtype,
                             device=self.buf.device)
            nb[:, :, :self.len] = self.buf[:, :, :self.len]
            self.buf = nb

    def drop_front(self, n: int):
        keep = self.buf[:, :, n:self.len].clone()
        self.len -= n
        self.buf[:, :, :self.len] = keep

    @staticmethod
    def drop_front_pair(k_w: "Window", v_w: "Window", n: int):
        """Slide both windows by n rows with one launch (the rows that stay -- residual_length of them -- move to the front)."""
        keep = k_w.len - n
        if v_w.len != k_w.len or k_w.buf.shape != v_w.buf.shape or not k_w.buf.is_cuda:
            k_w.drop_front(n)
            v_w.drop_front(n)
            return
        L = _lib.load()
        B, H, cap, D = k_w.buf.shape
        with torch.cuda.device(k_w.buf.device):
            err = L.mustafar_window_drop_front(torch.cuda.current_stream(k_w.buf.device).cuda_stream, k_w.buf.data_ptr(), v_w.buf.data_ptr(),
                                               cap * D, B * H, k_w.len, n)
        _lib.check(err, "mustafar_window_drop_front")
        k_w.len = v_w.len = keep

    def clone(self) -> "Window":
        w = Window.__new__(Window)
        w.buf, w.len = self.buf.clone(), self.len
        return w


class MustafarAttention:
    """Prefill + decode attention over the Mustafar cache (no projections, no RoPE: q/k/v arrive post-RoPE)."""

    def __init__(self, config: MustafarConfig):
        self.cfg = config
        self.num_heads = config.num_attention_heads
        self.num_key_value_heads = config.num_key_value_heads
        self.num_key_value_groups = self.num_heads // self.num_key_value_heads
        self.head_dim = config.head_dim
        if config.head_dim == 64 and (config.api != "fused" or config.arena):
            # the reference SpMV entry points are head_dim 128 only; head_dim 64 decodes through its own fused kernel
            raise ValueError("head_dim 64 is supported with MustafarConfig(api='fused', arena=False) only "
                             f"(got api={config.api!r}, arena={config.arena})")
        if config.hd64_extents and not (config.head_dim == 64 and config.api == "fused" and not config.arena):
            raise ValueError("hd64_extents is the head_dim 64 cache that grows by extents: it needs "
                             f"MustafarConfig(head_dim=64, api='fused', arena=False) (got head_dim={config.head_dim}, api={config.api!r}, "
                             f"arena={config.arena})")
        if config.hd64_raw_prefill and not (config.head_dim == 64 and config.api == "fused" and not config.arena):
            raise ValueError("hd64_raw_prefill is the head_dim 64 prefill compressed from the raw rows: it needs "
                             f"MustafarConfig(head_dim=64, api='fused', arena=False) (got head_dim={config.head_dim}, api={config.api!r}, "
                             f"arena={config.arena})")
        self.Reduction_Workspace = None   # model :658: a 1-element fp16 tensor shared by all layers

    # ---- pruning (model :77-153) -----------------------------------------------------------------------------
    def dh_prune_key(self, key_states: torch.Tensor, target_sparsity=None) -> torch.Tensor:
        return compression.prune_magnitude(key_states, self.cfg.k_sparsity if target_sparsity is None else target_sparsity)

    def dh_prune_value(self, value_states: torch.Tensor, target_sparsity=None) -> torch.Tensor:
        return compression.prune_magnitude(value_states, self.cfg.v_sparsity if target_sparsity is None else target_sparsity)

    def _slack(self) -> float:
        """Margin an arena is housed with: none where the cache grows by extents (nothing is ever appended in place), the
        configured one where a trigger appends in place (other GQA shapes, two launches asked for)."""
        cfg = self.cfg
        if cfg.extents and self._reads_extents(32):
            return 0.0
        return cfg.arena_slack

    def _flags(self) -> int:
        """`flags` of every fused call of this instance: its FMA engine and launch structure (MUSTAFAR_FLAG_* in include/mustafar_hip.h)."""
        return _lib.ENGINE_FLAGS[self.cfg.engine] | _lib.STRUCTURE_FLAGS[self.cfg.structure]

    def _reads_extents(self, columns: int) -> bool:
        """Whether this instance's launch form reads a cache that grows by extents, for scores of `columns` columns (compressed tokens +
        window capacity)."""
        return bool(_lib.load().mustafar_decode_reads_extents(self.num_key_value_groups, _ld_scores(columns), self._flags()))

    # ---- the base forms of an arena (cache.BaseForm: token rows of a key base, channel lists of a value base) ----------
    def _reads_form(self, cache, T: int, ld: int, flags: Optional[int] = None, form: Optional[BaseForm] = None) -> bool:
        """Whether the launch of a fused call sized for `T` compressed tokens, with scores of pitch `ld`, reads the base of arena `cache`
        in `form` (default: the form it is held in)."""
        groups = self.num_key_value_groups
        if self.head_dim != 128 or groups % 4:
            return False
        reads = getattr(_lib.load(), (form or cache.form).reads)
        return bool(reads(groups, T, cache.heads * (groups // 4), ld, self._flags() if flags is None else flags))

    def _wants_form(self, form: BaseForm) -> bool:
        cfg = self.cfg
        if form is VALUE_PAIR_LISTS and not self._wants_form(VALUE_LISTS):   # (the knob of the lists rules both list forms)
            return False
        if form is KEY_NIBBLE_ROWS and not (self._wants_form(KEY_ROWS) and self._wants_form(VALUE_PAIR_LISTS)):   # (read next to pair lists only)
            return False
        return getattr(cfg, form.name) is not False and os.environ.get("MUSTAFAR_" + form.name.upper(), "1") != "0" and cfg.head_dim == 128 and \
            self.num_key_value_groups % 4 == 0 and cfg.engine in ("valu", "fma_mix", "dot2", None, "default")

    def _retile_where_read(self, cache, window, form: BaseForm) -> None:
        """The ONE place that retiles a base into a form (to_fused()): where the launch of this cache's call shape reads it."""
        if isinstance(cache, CompressedArena) and cache.form is None and not cache.keep_tiles and self._wants_form(form) and \
                not torch.cuda.is_current_stream_capturing():
            T = cache.total_tokens
            if T and self._reads_form(cache, T, _ld_scores(T + window.cap), form=form):
                cache._retile(form)

    def _tiles_unless_read(self, cache, T: int, ops) -> None:
        """Tiles, unless the launch of the call at hand (`ops`, sized for `T` compressed tokens) reads the form `cache` is held in.
        (`require_tiles()` raises under capture.)"""
        if isinstance(cache, CompressedArena) and cache.form is not None and not self._reads_form(cache, T, ops.ld, ops.flags):
            cache.require_tiles()

    def _tiles_unless_read_pair(self, k, v, T: int, ops) -> None:
        """`_tiles_unless_read()` of both sides; nibble rows of a key base are read next to a value base in pair lists only."""
        self._tiles_unless_read(k, T, ops)
        self._tiles_unless_read(v, T, ops)
        if isinstance(k, CompressedArena) and k.form is KEY_NIBBLE_ROWS and getattr(v, "form", None) is not VALUE_PAIR_LISTS:
            k.require_tiles()

    def _kth(self, D: int) -> Tuple[int, int]:
        """`(kth_k, kth_v)`: the prune rule's kth (model :97) for K and V rows of D channels at the configured sparsities."""
        return compression.kth_from_sparsity(self.cfg.k_sparsity, D), compression.kth_from_sparsity(self.cfg.v_sparsity, D)

    def _compress_front(self, k_rows: torch.Tensor, v_rows: torch.Tensor):
        """The reference's trigger body on rows [0, 256) of a K and a V window [B, Hkv, >= 256, D]: prune (:325-326), compress
        (:328-337) -> `(k_new, v_new)`, two reference-layout caches of 256 tokens."""
        Bkv, D = k_rows.shape[0] * k_rows.shape[1], k_rows.shape[3]
        k_blk = self.dh_prune_key(k_rows[:, :, :256, :]).reshape(Bkv, -1, D)                             # :325
        v_blk = self.dh_prune_value(v_rows[:, :, :256, :]).reshape(Bkv, -1, D)                           # :326
        return _compress(k_blk, "key"), _compress(v_blk, "value")                                       # :328-337

    def _ws(self, device):
        if self.Reduction_Workspace is None or self.Reduction_Workspace.device != device:
            self.Reduction_Workspace = torch.zeros(1, dtype=torch.float16, device=device)
        return self.Reduction_Workspace

    # ---- prefill (model :405-445) ----------------------------------------------------------------------------
    def build_cache(self, key_states, value_states):
        """The cache-construction half of prefill (model :416-445): k/v [B,Hkv,L,D] fp16 -> past."""
        bsz, _, kv_seq_len, D = key_states.shape
        total_batch_kv = bsz * self.num_key_value_heads
        # :416 computes ((L - R)//256)*256, which is -256 for L < R; clamp at 0.
        compressed_length = max(0, ((kv_seq_len - self.cfg.residual_length) // 256) * 256)
        if compressed_length == 0:
            return Past(None, key_states, None, value_states, 0, kv_seq_len)
        arena = self.cfg.arena and self.cfg.api == "fused"
        if arena or self.cfg.hd64_raw_prefill:
            # In the model K and V arrive as transpose(1, 2) views of [B, L, H, D] projections (model :224-226; RoPE keeps the
            # strides): the kernels read rows of D contiguous halfs per head, so such views are made contiguous first.
            ks = key_states if key_states.is_contiguous() else key_states.contiguous()
            vs = value_states if value_states.is_contiguous() else value_states.contiguous()
            if arena:
                # straight from the raw K / V into appendable storage: prune thresholds in registers, no pruned copy (:419-434)
                k_compressed, v_compressed = CompressedArena.from_raw_pair(ks, vs, compressed_length, *self._kth(D), None, self._slack())
            else:
                # head_dim 64 from the raw rows: one chunked compression launch, one host wait, one gather per side
                k_compressed, v_compressed = compress_raw_pair_hd64(ks, vs, compressed_length, *self._kth(D))
            del ks, vs
        else:
            k_pruned = self.dh_prune_key(key_states[:, :, :compressed_length, :])                     # :419
            v_pruned = self.dh_prune_value(value_states[:, :, :compressed_length, :])                 # :420
            k_compressed = _compress(k_pruned.reshape(total_batch_kv, -1, D), "key")                  # :422-426
            v_compressed = _compress(v_pruned.reshape(total_batch_kv, -1, D), "value")                # :430-434
        k_local_window = key_states[:, :, compressed_length:, :].clone().contiguous()                 # :427
        v_local_window = value_states[:, :, compressed_length:, :].clone().contiguous()               # :435
        return Past(k_compressed, k_local_window, v_compressed, v_local_window, compressed_length, kv_seq_len)   # :445

    def prefill(self, query_states, key_states, value_states):
        """q [B,Hq,L,D], k/v [B,Hkv,L,D] fp16 -> (attn_output [B,Hq,L,D], past)."""
        attn_output = F.scaled_dot_product_attention(                                # flash_attn_func, :410-413
            query_states, repeat_kv(key_states, self.num_key_value_groups),
            repeat_kv(value_states, self.num_key_value_groups), is_causal=True)
        return attn_output, self.build_cache(key_states, value_states)

    # ---- fused decode (extension) ---------------------------------------------------------------------------
    EXTENT_CACHE_64 = ExtentCache64   # the cache class of hd64_extents (tests subclass it with a small table)

    NIBBLE_ROWS_FROM = 2048   # compressed tokens per head from which MustafarConfig(key_nibble_rows=None) prefers nibble rows

    def to_fused(self, past):
        """Wrap the two local windows of a reference-layout `past` into appendable buffers."""
        k_c, k_w, v_c, v_w, C, L = past
        if self.cfg.hd64_extents and C and not isinstance(k_c, ExtentCache64):   # (creates the device tables: before any capture)
            Bkv = k_w.shape[0] * k_w.shape[1] if not isinstance(k_w, Window) else k_w.buf.shape[0] * k_w.buf.shape[1]
            k_c, v_c = self.EXTENT_CACHE_64(k_c, "key", Bkv, C), self.EXTENT_CACHE_64(v_c, "value", Bkv, C)
        if self.cfg.arena and C and not isinstance(k_c, CompressedArena):
            k_c = CompressedArena.from_reference(k_c, "key", C, None, self._slack())
            v_c = CompressedArena.from_reference(v_c, "value", C, None, self._slack())
        if self.cfg.extents and isinstance(k_c, CompressedArena):
            k_c.ext_table, v_c.ext_table   # (exist before any graph that names them is captured: see decode_fused)
        if not isinstance(k_w, Window):
            cap = self.cfg.residual_length + 256   # the longest window: the step that fires the trigger (model :324) holds R + 256 rows
            k_w, v_w = Window(k_w, cap), Window(v_w, cap)
        # the lists over pairs of blocks are preferred where key rows are wanted too, the configuration they were measured in:
        # a matter of the configuration and the knobs, not of the state of this key arena; an arena that took them is no longer in tiles
        # for the line below
        if self._wants_form(KEY_ROWS):
            self._retile_where_read(v_c, v_w, VALUE_PAIR_LISTS)
        self._retile_where_read(v_c, v_w, VALUE_LISTS)
        # the key base: nibble rows next to a value base that took the pair lists (the measured configuration), else rows with channel bytes
        if getattr(v_c, "form", None) is VALUE_PAIR_LISTS and (self.cfg.key_nibble_rows or k_c.total_tokens >= self.NIBBLE_ROWS_FROM):
            self._retile_where_read(k_c, k_w, KEY_NIBBLE_ROWS)
        self._retile_where_read(k_c, k_w, KEY_ROWS)
        return Past(k_c, k_w, v_c, v_w, C, L)

    @staticmethod
    def advance(past, n: int):
        """Account on the host for `n` graph replays of a decode_fused(step_counter=...) call."""
        k_c, k_w, v_c, v_w, C, L = past
        k_w.len += n
        v_w.len += n
        return Past(k_c, k_w, v_c, v_w, C, L + n)

    def _scratch(self, device, BH, ld, ws_bytes):
        """Score scratch and slab workspace of the fused entry point, one pair per (device, stream): calls on different
        streams may overlap, calls on one stream cannot."""
        key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        pool = self.__dict__.setdefault("_fused_scratch", {})
        sc, ws = pool.get(key, (None, None))
        # Grown geometrically (+ two 256-token triggers of headroom) and never freed while this object lives: a captured graph
        # of an earlier call keeps the old addresses (bench.py records the graph of the NEXT cache length while the current one
        # is still being replayed).  Geometric growth keeps the retired buffers a small multiple of the live one.
        if sc is None or sc.numel() < BH * ld:
            self.__dict__.setdefault("_retired_scratch", []).append(sc)
            sc = torch.empty(max(BH * (ld + 512), (sc.numel() * 5) // 4 if sc is not None else 0), dtype=torch.float16, device=device)
        if ws is None or ws.numel() < ws_bytes:
            self.__dict__.setdefault("_retired_scratch", []).append(ws)
            ws = torch.empty(max(ws_bytes + ws_bytes // 8, (ws.numel() * 5) // 4 if ws is not None else 0, 1 << 20), dtype=torch.uint8, device=device)
        pool[key] = (sc, ws)
        return sc, ws

    def _decode_operands(self, query_states, T, window=None, step_counter=None, mask=(None, 0)):
        """What every fused entry point takes behind its cache arguments (`_lib._DECODE_TAIL`: q ... flags) for a launch sized for `T`
        compressed tokens, with the scratch and the output it names.  window: `(k_window, v_window, k_new, v_new, window_len,
        window_capacity)`, or None for a window-less call: null pointers and zero lengths.  mask: what `mask_args` returned.
        Returns a `DecodeOperands`; its `keep` holds the tensors whose addresses the operands carry until the call is issued."""
        bsz, D = query_states.shape[0], query_states.shape[3]
        BH, groups = bsz * self.num_heads, self.num_key_value_groups
        dev = query_states.device
        L = _lib.load()
        # (the head_dim-64 kernel picks its own split; at head_dim 128 the _hd form is mustafar_decode_workspace_bytes)
        split = 1 if D == 64 or not T else L.mustafar_value_pick_split_k(128, 1, T, BH, groups)
        ws_bytes = L.mustafar_decode_workspace_bytes_hd(T, BH, groups, split, D)
        k_win, v_win, kn, vn, w_len, cap = window if window is not None else (None, None, None, None, 0, 0)
        ld, flags = _ld_scores(T + cap), self._flags()
        scores, ws = self._scratch(dev, BH, ld, ws_bytes)
        out = torch.empty((bsz, self.num_heads, 1, D), dtype=torch.float16, device=dev)
        q = query_states if query_states.is_contiguous() else query_states.contiguous()
        p = lambda t: t.data_ptr() if t is not None else None
        tail = (q.data_ptr(), p(k_win), p(v_win), p(kn), p(vn), w_len, cap, scores.data_ptr(), ld, out.data_ptr(), ws.data_ptr(),
                split, T, BH, groups, math.sqrt(D), p(step_counter), p(mask[0]), mask[1], self.num_heads, flags)
        return DecodeOperands(out, tail, (q, kn, vn, mask[0]), ld, flags)

    def _step_operands(self, query_states, key_states, value_states, k_w, v_w, T, kv_seq_len, step_counter, attention_mask):
        """`_decode_operands` of a decode step: reserves the step's row in both windows and checks the mask.  T: the compressed tokens
        the launch is sized for.  Returns `(operands, w_len)`."""
        w_len = k_w.len + 1
        k_w.reserve(w_len)
        v_w.reserve(w_len)
        if k_w.cap != v_w.cap:
            raise RuntimeError("key/value windows must have the same capacity")
        kn = key_states if key_states.is_contiguous() else key_states.contiguous()
        vn = value_states if value_states.is_contiguous() else value_states.contiguous()
        if query_states.shape[3] == 64 and kn.data_ptr() % 16:   # (the head_dim-64 kernel reads the new key row as 16-byte pieces)
            kn = kn.clone()
        # a replayed graph reads more columns as the window grows: up to the window capacity (the bound ld_scores gets too)
        mask = mask_args(attention_mask, query_states.shape[0], T + (w_len if step_counter is None else k_w.cap), query_states.device,
                         kv_seq_len, exact=step_counter is None)
        return self._decode_operands(query_states, T, (k_w.buf, v_w.buf, kn, vn, w_len, k_w.cap), step_counter, mask), w_len

    def decode_fused(self, query_states, key_states, value_states, past, step_counter: Optional[torch.Tensor] = None,
                     attention_mask: Optional[torch.Tensor] = None, t_device: Optional[torch.Tensor] = None,
                     t_capacity: Optional[int] = None, defer_trigger: bool = False, return_lse: bool = False):
        """Same contract as decode() with api="native"; windows are `Window` objects appended in place.

        `return_lse`: return `(out, lse, past)`, `lse` fp32 [bsz, num_heads] = the log-sum-exp of each row's scores as the softmax saw
        them (scaled, masked), written by the row kernel of the same call: what `partial.merge_states` needs to combine this output
        with attention over tokens this call did not read.  Every cache kind, eagerly and under capture.  At
        head_dim 128 the LSE comes from the one-pass forms: a call that would run two launches raises ValueError.

        `attention_mask` is the hook's additive mask [bsz, 1, 1, kv_seq_len] (model :293-301), applied inside the softmax
        kernel exactly as the model does (fp16 add, clamp at finfo.min).  Under graph replay (`step_counter`) the rows must
        be at least `compressed_length + window capacity` long (checked: a shorter mask raises): the kernels read the first
        `kv_seq_len` columns of each row, whatever the step.

        `step_counter` (int32 device tensor, optional) is added to the window length inside the kernels, so that a
        captured graph of this call can be replayed for consecutive steps (advance it with mustafar_counter_add once
        per step); the host-side lengths/`kv_seq_len` of the returned `past` then describe the FIRST replay and the
        256-token trigger is the caller's business (see bench.py).

        `defer_trigger`: a step that reaches the 256-token trigger (model :324) returns with its windows at R + 256 rows and the
        compression NOT run; the caller runs it for all layers at once with `run_triggers()` before the next step (round 4: one
        library call issues every layer's compression, one host read, no allocation when `prepare_triggers()` was called ahead).

        `t_device` (int32 device tensor) + `t_capacity` (graph replay only: `step_counter` is required with them): the compressed
        tokens IN USE as a device quantity and the capacity the launch is sized for (a cache that grows by extents only).  ONE captured graph of the call then serves every compressed
        length up to `t_capacity`: after a trigger (run eagerly, outside the graph) the caller adds 256 to `t_device` and takes
        256 off `step_counter` (tests/test_gpu_extents.py)."""
        lse = None
        if return_lse:
            self._lse_served(past[4] if t_capacity is None else t_capacity)
            lse = torch.empty((query_states.shape[0], self.num_heads), dtype=torch.float32, device=query_states.device)
        out, new = self._decode_fused(query_states, key_states, value_states, past, step_counter, attention_mask, t_device, t_capacity,
                                      defer_trigger, lse)
        return (out, lse, new) if return_lse else (out, new)

    def _lse_served(self, C: int) -> None:
        """The calls whose LSE the library refuses (mustafar_hip.h: the head_dim 128 forms that run two launches), named."""
        if self.head_dim != 128:
            return
        if C == 0:
            raise ValueError("decode_fused(return_lse=True): no compressed tokens yet -- a window-only call at head_dim 128 runs the "
                             "two-launch form, which has no LSE")
        if self.cfg.structure == "two_launch":
            raise ValueError("decode_fused(return_lse=True): MustafarConfig(structure='two_launch') has no LSE; the one-pass forms do")
        if self.cfg.structure is None and _lib.load().mustafar_get_onepass() == 0:
            raise ValueError("decode_fused(return_lse=True): the process default is the two-launch form (MUSTAFAR_ONEPASS=0 / "
                             "mustafar_set_onepass(0)), which has no LSE")

    def _decode_fused(self, query_states, key_states, value_states, past, step_counter, attention_mask, t_device, t_capacity,
                      defer_trigger, lse):
        """decode_fused over every cache kind (reference-layout lists, arenas, ExtentCache64).  lse: None (the plain entry points), or
        the tensor the row kernel fills."""
        cfg = self.cfg
        bsz, _, q_len, D = query_states.shape
        assert q_len == 1 and ((D == 128 and not cfg.hd64_extents) or (D == 64 and self.head_dim == 64))
        past = self.to_fused(past)
        k_c, k_w, v_c, v_w, C, _ = past
        use_arena = isinstance(k_c, CompressedArena)
        T = C   # the compressed tokens the launch is sized for
        if t_device is not None:   # the launch is sized for the capacity; the kernels read the tokens in use from `t_device`
            if step_counter is None:
                raise ValueError("decode_fused: t_device is for captured graphs and needs step_counter (an eager call passes neither)")
            if cfg.hd64_extents:
                if t_capacity is None or not isinstance(k_c, ExtentCache64) or t_capacity <= k_c.tokens or t_capacity < C or \
                        (t_capacity - k_c.tokens) % 256 or (t_capacity - k_c.tokens) // 256 > k_c.MAX_EXTENTS:
                    raise ValueError("decode_fused: t_device needs an extent cache and t_capacity = base tokens + a multiple of 256 (at most the "
                                     "table's entries), not below the compressed length")
            elif t_capacity is None or t_capacity < C or (t_capacity - C) % 256 or not use_arena or t_capacity <= k_c.tokens:
                raise ValueError("decode_fused: t_device needs an arena cache and t_capacity = compressed length + a multiple of 256, beyond the base tokens")
            T = t_capacity
        kv_seq_len = past.kv_seq_len + 1
        ops, w_len = self._step_operands(query_states, key_states, value_states, k_w, v_w, T, kv_seq_len, step_counter, attention_mask)
        if use_arena:
            if cfg.extents and (k_c._ext_table is None or v_c._ext_table is None):
                # the extent tables must exist BEFORE a graph that names them is captured: created inside a capture they would
                # live in the graph's pool and their zero-fill would be replayed over the entries with every step
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("decode_fused: extent tables missing under graph capture (to_fused() creates them)")
                k_c.ext_table, v_c.ext_table
            # the cache has grown by extents (or, under a capture ahead of a trigger, is about to)
            if T > k_c.tokens and not _lib.load().mustafar_decode_reads_extents(self.num_key_value_groups, ops.ld, ops.flags):
                # an engine / structure switch after the cache grew: this form reads ONE view -- one copy of the cache.  (Not
                # possible under a capture, nor for a graph captured ahead of a trigger, whose extent does not exist yet; and the
                # forms with an LSE read extents or nothing.)
                if lse is not None or torch.cuda.is_current_stream_capturing() or k_c.tokens + 256 * len(k_c.extents) < T or \
                        t_device is not None:
                    raise RuntimeError("decode_fused: this launch form cannot read a cache that grows by extents "
                                       "(MustafarConfig(extents=False), or consolidate() the arenas first)")
                k_c, v_c = k_c.consolidate(), v_c.consolidate()   # (T == their base tokens now: the view form)
                k_c.ext_table, v_c.ext_table
                past = past._replace(k_cache=k_c, v_cache=v_c)
            self._tiles_unless_read_pair(k_c, v_c, T, ops)
        _call_decode(k_c, v_c, T, ops, D, t_device, lse)
        out = ops.out
        if step_counter is not None:
            return out, past   # lengths advance with the device counter
        k_w.len = v_w.len = w_len
        return out, self._close_step(Past(k_c, k_w, v_c, v_w, C, kv_seq_len), defer_trigger)

    def _close_step(self, new, defer_trigger: bool):
        """The tail of a fused step whose rows are appended and counted in `new`: the 256-token trigger (model :324-398) when it is due,
        or nothing with `defer_trigger` (run_triggers() then).  Returns the past to hand back."""
        cfg = self.cfg
        k_c, k_w, v_c, v_w, C = new[:5]
        use_arena = isinstance(k_c, CompressedArena)
        if defer_trigger:
            # run_triggers() works on arena and extent caches (a first trigger, C == 0, makes an arena when cfg.arena says so): anything
            # else would come back with a cache of the wrong kind, or fail inside run_triggers -- refuse here
            if not (cfg.hd64_extents or use_arena or (cfg.arena and C == 0)):
                raise RuntimeError("decode_fused(defer_trigger=True) needs an arena cache (MustafarConfig(arena=True)); "
                                   "tuple caches run their trigger inside the step")
            return new
        if not self.trigger_due(new):                                                                   # :324
            return new
        if cfg.hd64_extents:
            return self._run_triggers_ext64([new])[0]
        D = k_w.buf.shape[3]
        if use_arena or (cfg.arena and C == 0):
            # prune (:325-326) + compress + append (:328-390) of the raw window rows in one launch
            return self._trigger_one(new, *self._kth(D))
        Bkv = k_w.buf.shape[0] * k_w.buf.shape[1]
        k_new, v_new = self._compress_front(k_w.buf, v_w.buf)
        if C == 0:
            k_c, v_c = k_new, v_new
        else:
            k_c = append_compressed(k_c, k_new, Bkv, C, 256, D)
            v_c = append_compressed(v_c, v_new, Bkv, C, 256, D)
        k_w.drop_front(256)                                                                             # :392-393
        v_w.drop_front(256)
        return new._replace(k_cache=k_c, v_cache=v_c, compressed_length=C + 256)

    # ---- several query tokens per call (multi_query.hip) ------------------------------------------------------------
    def fits_before_trigger(self, past, n_q: int) -> int:
        """The largest n <= n_q such that no row but the last of an n-token call reaches a trigger point (`trigger_due`).  A caller that
        replays a graph of a fixed n_q asks before every replay: below n_q, it issues an eager call of that many tokens instead."""
        _, k_w, _, _, C, L = past
        w_len = k_w.len if isinstance(k_w, Window) else k_w.shape[2]
        for j in range(n_q - 1):
            if (L + j + 1 - self.cfg.residual_length - C) % 256 == 0 and w_len + j + 1 >= 256:
                return j + 1
        return n_q

    _fits_before_trigger = fits_before_trigger   # compatibility alias only (the name before it was public): not a second API

    @staticmethod
    def _device_int(t, name: str, dev) -> None:
        """A device-side length as the kernels load it: ONE int32 on the query's device (its address goes to the library as it is)."""
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.numel() != 1 or t.device != dev:
            raise ValueError(f"decode_multi: {name} must be an int32 tensor of one element on the device of the query ({dev}); got "
                             f"{(t.dtype, tuple(t.shape), str(t.device)) if isinstance(t, torch.Tensor) else type(t).__name__}")

    @staticmethod
    def _multi_mask(attention_mask, bsz: int, n_q: int, columns: int, dev, exact: bool = True):
        """The additive fp16 mask of a decode_multi call, checked: [bsz, 1, 1 or n_q, columns] on `dev` (not `exact`, a replayed graph:
        at least `columns`), rows and planes at least `columns` halfs apart and unit stride along a row (made contiguous otherwise); or
        None."""
        if attention_mask is None:
            return None
        if attention_mask.dim() != 4 or attention_mask.shape[:2] != (bsz, 1) or attention_mask.shape[2] not in (1, n_q) or \
                attention_mask.shape[3] < columns or (exact and attention_mask.shape[3] != columns):
            raise ValueError(f"Attention mask should be of size {(bsz, 1, n_q, columns)} or {(bsz, 1, 1, columns)}, but is "
                             f"{tuple(attention_mask.size())}")
        if attention_mask.dtype != torch.float16 or attention_mask.device != dev:
            raise RuntimeError("attention_mask must be a float16 tensor on the device of the query")
        if attention_mask.stride(3) != 1 or (bsz > 1 and attention_mask.stride(0) < columns) or \
                (attention_mask.shape[2] > 1 and attention_mask.stride(2) < columns):
            attention_mask = attention_mask.contiguous()
        return attention_mask

    def _multi_shapes(self, what: str, query_states, key_states, value_states) -> int:
        """The configuration and the shapes a several-token call over the live cache takes (`what`: the method the errors name) -> n_q."""
        if self.cfg.api != "fused":
            raise ValueError(f"{what} needs MustafarConfig(api='fused')")
        groups = self.num_key_value_groups
        if groups > 8:
            raise ValueError(f"{what} serves 1 to 8 q heads per kv head (got {groups})")
        if query_states.dim() != 4:
            raise ValueError(f"{what}: q [bsz, {self.num_heads}, n_q, {self.head_dim}] (got {tuple(query_states.shape)})")
        bsz, H, n_q, D = query_states.shape
        if H != self.num_heads or D != self.head_dim or n_q < 1 or key_states.shape != (bsz, self.num_key_value_heads, n_q, D) or \
                value_states.shape != key_states.shape:
            raise ValueError(f"{what}: q [bsz, {self.num_heads}, n_q, {self.head_dim}] with k / v [bsz, {self.num_key_value_heads}, n_q, "
                             f"{self.head_dim}] (got {tuple(query_states.shape)}, {tuple(key_states.shape)}, {tuple(value_states.shape)})")
        return n_q

    def _multi_fits(self, what: str, past, n_q: int) -> None:
        """The trigger-point rule of a several-token call: a trigger point may only be its last row."""
        fits = self.fits_before_trigger(past, n_q)
        if fits < n_q:
            raise ValueError(f"{what}: {n_q} tokens would step over a 256-token trigger point; at most {fits} fit in this call "
                             "(the trigger point may only be the last row: accept() then runs the trigger)")

    def decode_multi(self, query_states, key_states, value_states, past, return_lse: bool = False, attention_mask=None,
                     step_counter: Optional[torch.Tensor] = None, t_device: Optional[torch.Tensor] = None,
                     t_capacity: Optional[int] = None):
        """n_q consecutive tokens of every sequence in one call: q [bsz, H, n_q, D], their new k / v [bsz, Hkv, n_q, D] -> (out
        [bsz, H, n_q, D], past'), or (out, lse fp32 [bsz, H, n_q], past') with `return_lse`.  Token j attends to the cache, the window
        and the new rows 0 .. j: what n_q decode_fused steps compute, with the compressed cache read once (speculative decoding, a short
        follow-up turn).  Needs api="fused"; every cache kind decode_fused serves at this head dim (reference-layout lists, arenas with
        extents or in place, ExtentCache64, nothing compressed yet); 1 to 8 q heads per kv head.  More than 64 // groups tokens run as
        consecutive calls of at most that many.

        The call appends the rows and never compresses: close it with `accept()`, which drops the rejected rows and runs the 256-token
        trigger when it is due.  A trigger point may only be the LAST row of a call -- a call that would step over one raises ValueError
        naming the largest n_q that fits.

        attention_mask: additive fp16 on the query's device, [bsz, 1, 1 or n_q, kv_seq_len + n_q] (one plane per sequence).  Row j of an
        [.., n_q, ..] mask is what a decode_fused step for token j would get as mask[:, :, j:j+1, :kv_seq_len + j + 1] -- HF's 4-D form
        with its finfo.min upper triangle among the new tokens works unchanged; the causal limit holds whatever the mask says, so a mask
        only takes columns away: left padding, the holes of a batch whose sequences accepted different numbers of drafts, or a draft
        tree (0 on a node's ancestors and itself, finfo.min on the other new tokens; close with accept(keep=path)).  INTEGRATION.md 5.

        `step_counter`, `t_device`, `t_capacity`: as in decode_fused, for ONE captured graph of the call replayed while the cache grows.
        `step_counter` (int32 device tensor) is added to the window length inside the kernels; the returned past keeps the host lengths
        of the FIRST replay, and the caller accounts with `advance(past, n_q)` before `accept()` and adds the rows that stayed to the
        counter (mustafar_counter_add).  The windows must already have their full capacity (a past from `to_fused()` has), n_q must fit
        one library call (n_q <= 64 // groups), and a mask is [bsz, 1, 1 or n_q, >= compressed capacity + window capacity], refilled by
        the caller between replays: window row w sits at column compressed-tokens-in-use + w.  `t_device` (int32 device tensor, with
        `step_counter`) holds the compressed tokens in use and `t_capacity` the tokens the launch is sized for (an arena that grows by
        extents, or an ExtentCache64): after a trigger, run eagerly, the caller adds 256 to `t_device` and takes 256 off the counter.
        `fits_before_trigger(past, n_q)` says when a replay would step over a trigger point."""
        groups = self.num_key_value_groups
        n_q = self._multi_shapes("decode_multi", query_states, key_states, value_states)
        per = 64 // groups
        if t_device is not None and step_counter is None:
            raise ValueError("decode_multi: t_device is for captured graphs and needs step_counter (an eager call passes neither)")
        if step_counter is not None:
            self._device_int(step_counter, "step_counter", query_states.device)
        if t_device is not None:
            self._device_int(t_device, "t_device", query_states.device)
        if step_counter is not None and n_q > per:
            raise ValueError(f"decode_multi: a replayed call (step_counter) is one library call: at most {per} tokens at {groups} q heads "
                             f"per kv head (got {n_q})")
        self._multi_fits("decode_multi", past, n_q)
        if step_counter is not None:
            return self._decode_multi_replayed(query_states, key_states, value_states, past, return_lse, attention_mask, step_counter,
                                               t_device, t_capacity)
        out, lse, past = self._decode_multi_eager(query_states, key_states, value_states, past, attention_mask)
        return (out, lse, past) if return_lse else (out, past)

    def _decode_multi_eager(self, query_states, key_states, value_states, past, attention_mask, out=None, lse=None):
        """The eager body of decode_multi behind its checks: consecutive library calls of at most 64 // groups tokens -> (out, lse, past').
        out / lse (decode_multi_split): contiguous [bsz, H, n_q, D] fp16 / [bsz, H, n_q] fp32 that take the result -- a single library
        call writes them itself, the pieces of several are copied in."""
        bsz, _, n_q, _ = query_states.shape
        per = 64 // self.num_key_value_groups
        kv_seq_len = Past(*past).kv_seq_len
        mask = self._multi_mask(attention_mask, bsz, n_q, kv_seq_len + n_q, query_states.device)
        past = self.to_fused(past)
        if n_q <= per:
            return self._decode_multi_call(query_states, key_states, value_states, past, mask, out=out, lse=lse)
        outs, lses = [], []
        for s0 in range(0, n_q, per):
            s1 = min(n_q, s0 + per)
            m = None
            if mask is not None:   # the sub-call's rows, and the columns up to its last new row
                m = mask[:, :, (s0 if mask.shape[2] > 1 else 0):(s1 if mask.shape[2] > 1 else 1), :kv_seq_len + s1]
            o, l, past = self._decode_multi_call(query_states[:, :, s0:s1], key_states[:, :, s0:s1], value_states[:, :, s0:s1], past, m)
            outs.append(o)
            lses.append(l)
        if out is None:
            return torch.cat(outs, dim=2), torch.cat(lses, dim=2), past
        torch.cat(outs, dim=2, out=out)
        torch.cat(lses, dim=2, out=lse)
        return out, lse, past

    def _decode_multi_replayed(self, query_states, key_states, value_states, past, return_lse, attention_mask, step_counter, t_device,
                               t_capacity):
        """decode_multi with `step_counter`: the checks a graph that outlives this call needs, then ONE library call whose lengths come
        from the device.  The returned past is the one that came in (as a fused past): the host lengths of the first replay."""
        cfg = self.cfg
        bsz, _, n_q, _ = query_states.shape
        past = self.to_fused(past)
        k_c, k_w, v_c, v_w, C, _ = past
        full = cfg.residual_length + 256   # the longest window: the step that fires the trigger holds R + 256 rows (to_fused)
        if k_w.cap < full or v_w.cap != k_w.cap or k_w.len + n_q > k_w.cap:
            raise ValueError(f"decode_multi: under graph replay (step_counter) the windows must already have their full capacity of "
                             f"{full} rows and room for this call -- a graph keeps their addresses, nothing may be reallocated (got "
                             f"{k_w.cap} / {v_w.cap} rows of capacity, {k_w.len} in use, {n_q} new)")
        T = C   # the compressed tokens the launch is sized for
        if t_device is not None:
            if cfg.hd64_extents:
                if t_capacity is None or not isinstance(k_c, ExtentCache64) or t_capacity <= k_c.tokens or t_capacity < C or \
                        (t_capacity - k_c.tokens) % 256 or (t_capacity - k_c.tokens) // 256 > k_c.MAX_EXTENTS:
                    raise ValueError("decode_multi: t_device needs an extent cache and t_capacity = base tokens + a multiple of 256 (at most the "
                                     "table's entries), not below the compressed length")
            elif t_capacity is None or t_capacity < C or (t_capacity - C) % 256 or not isinstance(k_c, CompressedArena) or \
                    not cfg.extents or t_capacity <= k_c.tokens or (t_capacity - k_c.tokens) // 256 > k_c.MAX_EXTENTS:
                raise ValueError("decode_multi: t_device needs an arena cache that grows by extents and t_capacity = compressed length + a "
                                 "multiple of 256, beyond the base tokens")
            T = t_capacity
        elif t_capacity is not None:
            raise ValueError("decode_multi: t_capacity goes with t_device (the compressed tokens in use, on the device)")
        # a replayed graph reads more columns as the cache and the window grow: up to the two capacities
        mask = self._multi_mask(attention_mask, bsz, n_q, T + k_w.cap, query_states.device, exact=False)
        out, lse, past = self._decode_multi_call(query_states, key_states, value_states, past, mask, step_counter, t_device, T)
        return (out, lse, past) if return_lse else (out, past)

    def _decode_multi_call(self, q, k_rows, v_rows, past, mask=None, step_counter=None, t_device=None, T=None, out=None, lse=None):
        """One mustafar_decode_multi_query(_masked, _lengths) call: at most 64 // groups tokens, appended to the windows and counted in the
        returned past.  mask: None, or a checked view [bsz, 1, 1 or n, kv_seq_len + n] (`_multi_mask`) whose address and strides the call
        takes.  step_counter / t_device (`_decode_multi_replayed`): the lengths come from the device, the launch is sized for `T`
        compressed tokens and the window capacity, nothing is reallocated and the past comes back with the host lengths it had.
        out / lse: the contiguous tensors the call writes (decode_multi_split's slices), or None: allocated here."""
        past = Past(*past)
        k_c, k_w, v_c, v_w, C = past[:5]
        T = C if T is None else T
        bsz, H, n, D = q.shape
        Bkv, groups, dev = bsz * self.num_key_value_heads, self.num_key_value_groups, q.device
        w_len = k_w.len + n
        if step_counter is None:
            k_w.reserve(w_len)
            v_w.reserve(w_len)
        if k_w.cap != v_w.cap or k_w.len != v_w.len:
            raise RuntimeError("key/value windows must have the same length and capacity")
        q = q.contiguous()
        kn, vn = k_rows.contiguous(), v_rows.contiguous()
        k = as_cache(k_c, C)   # (an arena is poll()ed by view_args; an ExtentCache64 always names its tables here)
        (kv, vv, t_base, kt, vt), keep = k.view_args(as_cache(v_c, C), tables=T > k.tokens or k.lse_reads_tables)
        L = _lib.load()
        ws_bytes = L.mustafar_decode_multi_query_workspace_bytes(T, k_w.cap, Bkv, groups, n, D)
        if ws_bytes <= 0:
            raise ValueError(f"decode_multi: the library serves no call of {n} tokens x {groups} q heads per kv head, {T} compressed tokens, "
                             f"a window of {k_w.cap} rows, head_dim {D}")
        _, ws = self._scratch(dev, 0, 0, ws_bytes)
        if out is None:
            out = torch.empty((bsz, H, n, D), dtype=torch.float16, device=dev)
            lse = torch.empty((bsz, H, n), dtype=torch.float32, device=dev)
        args = (kv, vv, t_base, kt, vt, T, Bkv, groups, n, q.data_ptr(), k_w.buf.data_ptr(), v_w.buf.data_ptr(), kn.data_ptr(), vn.data_ptr(),
                w_len, k_w.cap, out.data_ptr(), lse.data_ptr(), ws.data_ptr(), math.sqrt(D), D)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            margs = (None, 0, 0, 1, 1)
            if mask is not None:   # one plane per sequence: its kv heads share it
                margs = (mask.data_ptr(), mask.stride(0), mask.stride(2), mask.shape[2], self.num_key_value_heads)
            if step_counter is not None:
                err = L.mustafar_decode_multi_query_lengths(st, *args, *margs, step_counter.data_ptr(),
                                                            t_device.data_ptr() if t_device is not None else None)
            elif mask is None:
                err = L.mustafar_decode_multi_query(st, *args)
            else:
                err = L.mustafar_decode_multi_query_masked(st, *args, *margs)
        _lib.check(err, "mustafar_decode_multi_query")
        del keep   # (alive until here: the call has been issued)
        if step_counter is not None:
            return out, lse, past   # lengths advance with the device counter
        k_w.len = v_w.len = w_len
        return out, lse, past._replace(kv_seq_len=past.kv_seq_len + n)

    # ---- ragged batches: independent bsz-1 pasts in one call (ragged.py, ragged_batch.hip) ------------------------------
    def decode_ragged(self, query_states, key_states, value_states, pasts, return_lse: bool = False, batch: Optional[RaggedBatch] = None):
        """n_q consecutive tokens of each of n sequences that share nothing but this attention object: q [n, H, n_q, D], their new k / v
        [n, Hkv, n_q, D] and `pasts`, a list of n bsz-1 pasts (any cache kind decode_multi serves, mixed freely) -> (out [n, H, n_q, D],
        pasts'), or (out, lse fp32 [n, H, n_q], pasts') with `return_lse`.  One library call reads only the tokens that exist: no
        padding, no mask; sequence s gets bit for bit what decode_multi on its past alone returns.  Close the call per sequence with
        `accept(pasts'[s], rejected=r_s)` or `accept(pasts'[s], keep=, n_q=)`: each sequence drops its own number of drafts and runs its
        own 256-token trigger when it is due.  `batch`: the `ragged.RaggedBatch` whose device table the call uses; None: one of this
        object's own, made at the first call (outside any graph capture) and grown when a call brings more sequences.  ValueError as
        `RaggedBatch.decode` lists them; n_q is limited to 64 // groups, one library call.  INTEGRATION.md 5."""
        if batch is None:
            if self.cfg.api != "fused":
                raise ValueError("decode_ragged needs MustafarConfig(api='fused')")
            batch = self.__dict__.get("_ragged_batch")
            if batch is None or batch.capacity < len(pasts):
                batch = self._ragged_batch = RaggedBatch(self, max(len(pasts), 8))
        return batch.decode(query_states, key_states, value_states, pasts, return_lse)

    def accept(self, past, rejected: int = 0, defer_trigger: bool = False, keep=None, n_q: Optional[int] = None):
        """Close a decode_multi call: drop the `rejected` newest rows (0 <= rejected < the rows the window holds) -- only the host lengths
        change, the rows stay in the buffer and the next append overwrites them -- then run the 256-token trigger exactly as a decode_fused
        step does when it is due.  `defer_trigger`: return with the trigger not run, for run_triggers() over all layers.

        keep (with n_q, the tokens of the last call; not with `rejected`): an integer tensor [bsz, n_keep] of indices into those n_q rows,
        per sequence -- the accepted path of a draft tree, or the accepted prefix padded with any rejected node where a sequence accepted
        less than the longest.  The rows are gathered to the front of the n_q rows of both windows (mustafar_window_keep_rows: one launch,
        any order, duplicates allowed, indices clamped to [0, n_q)), the lengths become len - n_q + n_keep, then the trigger as above."""
        past = Past(*past)
        k_w, v_w = past.k_window, past.v_window
        if not isinstance(k_w, Window) or not isinstance(v_w, Window):
            raise ValueError("accept() closes a decode_multi call: the past it returned (windows in appendable buffers)")
        if keep is not None:
            if rejected != 0:
                raise ValueError("accept: keep= says which rows stay; it does not go with rejected != 0")
            if n_q is None:
                raise ValueError("accept: keep= needs n_q, the number of tokens of the decode_multi call it closes")
            if not 1 <= n_q <= min(k_w.len, v_w.len, 64) or k_w.len != v_w.len or k_w.buf.shape != v_w.buf.shape:
                raise ValueError(f"accept: n_q must be in [1, {min(k_w.len, v_w.len, 64)}] -- the rows of one call, in windows of equal "
                                 f"length and capacity (got {n_q}; the windows hold {k_w.len} / {v_w.len} rows)")
            bsz = k_w.buf.shape[0]
            if not isinstance(keep, torch.Tensor) or keep.dtype.is_floating_point or keep.dtype == torch.bool or keep.dim() != 2 or \
                    keep.shape[0] != bsz or not 1 <= keep.shape[1] <= n_q:
                raise ValueError(f"accept: keep must be an integer tensor [{bsz}, 1..{n_q}] of indices into the {n_q} rows of the last call "
                                 f"(got {tuple(keep.shape) if isinstance(keep, torch.Tensor) else type(keep).__name__})")
            n_keep, dev = keep.shape[1], k_w.buf.device
            idx = keep.to(device=dev, dtype=torch.int32).contiguous()
            B, Hkv, cap, D = k_w.buf.shape
            with torch.cuda.device(dev):
                err = _lib.load().mustafar_window_keep_rows(torch.cuda.current_stream(dev).cuda_stream, k_w.buf.data_ptr(), v_w.buf.data_ptr(),
                                                            B * Hkv, Hkv, cap, D, k_w.len - n_q, n_q, idx.data_ptr(), n_keep)
            _lib.check(err, "mustafar_window_keep_rows")
            del idx   # (alive until here: the call has been issued)
            rejected = n_q - n_keep
        if not 0 <= rejected < min(k_w.len, v_w.len):
            raise ValueError(f"accept: rejected must be in [0, {min(k_w.len, v_w.len)}) -- the window holds {k_w.len} rows (got {rejected})")
        k_w.len -= rejected
        v_w.len -= rejected
        return self._close_step(past._replace(kv_seq_len=past.kv_seq_len - rejected), defer_trigger)

    def decode_split(self, query_states, key_states, value_states, past, frozen, attention_mask=None):
        """One decode step over frozen compressed segments + the live cache: `frozen` is a list of `(k_cache, v_cache, tokens)` that
        precede the live cache in sequence order (partial.decode_segment says what a segment may be), and / or of
        `partial.SharedSegment`s -- one copy of kv_heads heads that every sequence of the batch reads (no mask then): anything that is not
        a tuple is taken for one, and asked for its `tokens` and to `decode(attn, q)`.  One window-less call per
        segment, one decode_fused(return_lse=True) call on `past`, one merge (merge_states).  `attention_mask`: additive fp16
        [bsz, 1, 1, frozen tokens + kv_seq_len]; every call reads its own columns (the pointer moves, rows need no alignment).
        Returns (out, past) with the contract of decode(); the 256-token trigger runs on the live cache only."""
        if self.cfg.api != "fused":
            raise ValueError("decode_split needs MustafarConfig(api='fused')")
        outs, lses, col = [], [], 0
        shared = [not isinstance(f, (tuple, list)) for f in frozen]
        if any(shared) and attention_mask is not None:
            raise ValueError("decode_split: a SharedSegment in `frozen` takes no attention mask (left padding and a shared prefix do not "
                             "coexist); pass attention_mask=None")
        total = sum(f.tokens if sh else int(f[2]) for f, sh in zip(frozen, shared)) + Past(*past).kv_seq_len + 1
        if attention_mask is not None and (attention_mask.dim() != 4 or attention_mask.shape[3] != total):
            raise ValueError(f"Attention mask should be of size {(query_states.shape[0], 1, 1, total)}, but is {tuple(attention_mask.size())}")
        for f, sh in zip(frozen, shared):
            if sh:   # one copy for the whole batch: mustafar_decode_shared_segment
                o, l = f.decode(self, query_states)
            else:
                k_cache, v_cache, tokens = f
                m = attention_mask[..., col:col + tokens] if attention_mask is not None else None
                o, l = self.decode_segment(query_states, k_cache, v_cache, tokens, m)
                col += tokens
            outs.append(o)
            lses.append(l)
        m = attention_mask[..., col:] if attention_mask is not None else None
        o, l, new = self.decode_fused(query_states, key_states, value_states, past, attention_mask=m, return_lse=True)
        outs.append(o)
        lses.append(l)
        out, _ = merge_states(outs, lses)
        return out, new

    def _segment_query(self, query_states) -> None:
        bsz, H, q_len, D = query_states.shape
        if q_len != 1 or H != self.num_heads or D != self.head_dim:
            raise ValueError(f"decode_segment: query of shape {tuple(query_states.shape)} for {self.num_heads} heads of {self.head_dim}")

    def decode_segment(self, query_states, k_cache, v_cache, tokens, attention_mask=None):
        """The window-less call of partial.decode_segment over one per-sequence segment (documented there)."""
        self._segment_query(query_states)
        bsz, H, _, D = query_states.shape
        if v_cache is None or tokens is None:
            raise ValueError("decode_segment: a per-sequence segment is (k_cache, v_cache, tokens)")
        if tokens <= 0 or tokens % 64:
            raise ValueError(f"decode_segment: a segment holds a positive multiple of 64 tokens (got {tokens})")
        if isinstance(k_cache, CompressedArena) and tokens % 256:
            # the extents entry points take an arena's base in whole 256-token blocks (mustafar_hip.h); the several-token segment call reads
            # any multiple of 64, so a shorter tail goes there as one token
            out, lse = self._decode_segment_multi(query_states, k_cache, v_cache, tokens, attention_mask)
            return out, lse.reshape(bsz, H)
        if D == 128:   # the LSE comes from the one-pass forms (mustafar_hip.h)
            self._lse_served(tokens)
        k, v = as_cache(k_cache, tokens), as_cache(v_cache, tokens)
        if type(k) is not type(v) or k.total_tokens != tokens or v.total_tokens != tokens:
            raise ValueError(f"decode_segment: the caches hold {k.total_tokens} / {v.total_tokens} tokens, not {tokens}")
        dev = query_states.device
        # no window argument at all: the window-less form of the entry points with an LSE; an arena's tables only when it has extents
        ops = self._decode_operands(query_states, tokens, mask=mask_args(attention_mask, bsz, tokens, dev))
        lse = torch.empty((bsz, H), dtype=torch.float32, device=dev)
        self._tiles_unless_read_pair(k, v, tokens, ops)
        _call_decode(k, v, tokens, ops, D, None, lse)
        return ops.out, lse

    # ---- several query tokens over frozen and shared segments -----------------------------------------------------------
    def _segment_query_multi(self, what: str, query_states) -> int:
        """What every several-token segment call checks first (`what`: the method the errors name) -> n_q."""
        if self.cfg.api != "fused":
            raise ValueError(f"{what} needs MustafarConfig(api='fused')")
        if self.num_key_value_groups > 8:
            raise ValueError(f"{what} serves 1 to 8 q heads per kv head (got {self.num_key_value_groups})")
        if query_states.dim() != 4 or query_states.shape[1] != self.num_heads or query_states.shape[3] != self.head_dim or \
                query_states.shape[2] < 1:
            raise ValueError(f"{what}: query of shape {tuple(query_states.shape)} for {self.num_heads} heads of {self.head_dim} "
                             f"([bsz, {self.num_heads}, n_q, {self.head_dim}], n_q >= 1)")
        return query_states.shape[2]

    def decode_segment_multi(self, query_states, k_cache, v_cache=None, tokens=None, attention_mask=None):
        """partial.decode_segment_multi (documented there): n_q query tokens of every sequence over ONE frozen segment."""
        return self._decode_segment_multi(query_states, k_cache, v_cache, tokens, attention_mask)

    def _decode_segment_multi(self, query_states, k_cache, v_cache, tokens, attention_mask, out=None, lse=None):
        """decode_segment_multi; out / lse (decode_multi_split): the contiguous [bsz, H, n_q, D] fp16 / [bsz, H, n_q] fp32 the call writes."""
        what = "decode_segment_multi"
        n_q = self._segment_query_multi(what, query_states)
        if hasattr(k_cache, "_decode_multi"):   # a partial.SharedSegment: one copy for the whole batch
            if v_cache is not None or tokens is not None:
                raise ValueError(f"{what}: a SharedSegment carries both caches and its token count")
            if attention_mask is not None:
                raise ValueError(f"{what}: a shared segment takes no attention mask: its one copy is visible to every row (decode_multi_split "
                                 "skips its columns)")
            return k_cache._decode_multi(self, query_states, out, lse)
        bsz, H, _, D = query_states.shape
        groups, Bkv = self.num_key_value_groups, bsz * self.num_key_value_heads
        if v_cache is None or tokens is None:
            raise ValueError(f"{what}: a per-sequence segment is (k_cache, v_cache, tokens)")
        if tokens <= 0 or tokens % 64:
            raise ValueError(f"{what}: a segment holds a positive multiple of 64 tokens (got {tokens})")
        if n_q * groups > 1024:
            raise ValueError(f"{what}: at most {1024 // groups} tokens per call at {groups} q heads per kv head (got {n_q})")
        dev = query_states.device
        mask = self._multi_mask(attention_mask, bsz, n_q, tokens, dev, exact=False)
        k, v = as_cache(k_cache, tokens), as_cache(v_cache, tokens)
        if type(k) is not type(v) or k.total_tokens != tokens or v.total_tokens != tokens:
            raise ValueError(f"{what}: the caches hold {k.total_tokens} / {v.total_tokens} tokens, not {tokens}")
        if query_states.dtype != torch.float16 or not query_states.is_cuda:
            raise ValueError(f"{what}: the query is a float16 tensor on the GPU (got {query_states.dtype} on {query_states.device})")
        q = query_states.contiguous()
        (kv, vv, t_base, kt, vt), keep = k.view_args(v, tables=tokens > k.tokens)   # (an arena is poll()ed, a key base in rows retiled)
        L = _lib.load()
        ws_bytes = L.mustafar_decode_multi_segment_workspace_bytes(tokens, Bkv, groups, n_q, D)
        if ws_bytes <= 0:
            raise ValueError(f"{what}: the library serves no call of {n_q} tokens x {groups} q heads per kv head over {tokens} tokens, head_dim {D}")
        _, ws = self._scratch(dev, 0, 0, ws_bytes)
        if out is None:
            out = torch.empty((bsz, H, n_q, D), dtype=torch.float16, device=dev)
            lse = torch.empty((bsz, H, n_q), dtype=torch.float32, device=dev)
        margs = (None, 0, 0, 1, 1)
        if mask is not None:   # one plane per sequence: its kv heads share it
            margs = (mask.data_ptr(), mask.stride(0), mask.stride(2), mask.shape[2], self.num_key_value_heads)
        with torch.cuda.device(dev):
            err = L.mustafar_decode_multi_segment(torch.cuda.current_stream(dev).cuda_stream, kv, vv, t_base, kt, vt, tokens, Bkv, groups, n_q,
                                                  q.data_ptr(), out.data_ptr(), lse.data_ptr(), ws.data_ptr(), math.sqrt(D), D, *margs)
        _lib.check(err, "mustafar_decode_multi_segment")
        del keep, q, mask   # (alive until here: the call has been issued)
        return out, lse

    def decode_multi_split(self, query_states, key_states, value_states, past, frozen, attention_mask=None, return_lse: bool = False):
        """decode_multi over frozen compressed segments + the live cache: n_q tokens of every sequence, q [bsz, H, n_q, D] with their new
        k / v [bsz, Hkv, n_q, D] -> (out [bsz, H, n_q, D], past'), or (out, lse fp32 [bsz, H, n_q], past') with `return_lse`.  `frozen` is
        what decode_split takes: `(k_cache, v_cache, tokens)` tuples that precede the live cache in sequence order and / or
        `partial.SharedSegment`s.  Every query token sees ALL tokens of every frozen entry (they precede the new tokens: no causal limit
        there) and the live cache as in decode_multi.  One call per frozen entry over all n_q tokens at once
        (mustafar_decode_shared_segment_multi / mustafar_decode_multi_segment), decode_multi(return_lse=True) on `past` -- its trigger-point
        rule and its chunking by 64 // groups tokens apply to the live call as they do there --, then ONE mustafar_merge_attention_states
        over the flat bsz * H * n_q rows.  The stacked outputs and LSEs of the parts are allocated once and every call writes its own slice.

        past': exactly what decode_multi returns for the live cache alone -- rows appended, nothing compressed: close it with `accept()`
        (rejected=, keep=, the trigger).

        attention_mask: additive fp16 [bsz, 1, 1 or n_q, frozen tokens + kv_seq_len + n_q], the frozen entries' columns first, in order
        (those of SharedSegments included).  Each per-sequence entry and the live call read their own column slice; the columns of a
        shared entry are NEVER read -- one copy is visible to every row --, so a draft tree or left padding in the live part works next
        to a shared prefix (decode_split refuses that combination and keeps doing so: there the mask has no columns for a shared entry).
        Device-side lengths (step_counter / t_device) are not taken: one captured graph serves fixed lengths."""
        what = "decode_multi_split"
        n_q = self._multi_shapes(what, query_states, key_states, value_states)
        bsz, H, _, D = query_states.shape
        past = Past(*past)
        frozen = list(frozen)
        if len(frozen) > 63:
            raise ValueError(f"{what}: at most 63 frozen entries (one merge of 64 parts; got {len(frozen)})")
        shared = [not isinstance(f, (tuple, list)) for f in frozen]
        tokens = [int(f.tokens) if sh else int(f[2]) for f, sh in zip(frozen, shared)]
        total = sum(tokens) + past.kv_seq_len + n_q
        if attention_mask is not None and (attention_mask.dim() != 4 or attention_mask.shape[:2] != (bsz, 1) or
                                           attention_mask.shape[2] not in (1, n_q) or attention_mask.shape[3] != total):
            raise ValueError(f"Attention mask should be of size {(bsz, 1, n_q, total)} or {(bsz, 1, 1, total)}, but is "
                             f"{tuple(attention_mask.size())}")
        self._multi_fits(what, past, n_q)
        dev, parts = query_states.device, len(frozen) + 1
        o_all = torch.empty((parts, bsz, H, n_q, D), dtype=torch.float16, device=dev)
        l_all = torch.empty((parts, bsz, H, n_q), dtype=torch.float32, device=dev)
        col = 0
        for i, (f, sh, t) in enumerate(zip(frozen, shared, tokens)):
            if sh:   # one copy for the whole batch; its mask columns are skipped
                f._decode_multi(self, query_states, o_all[i], l_all[i])
            else:
                m = attention_mask[..., col:col + t] if attention_mask is not None else None
                self._decode_segment_multi(query_states, f[0], f[1], t, m, o_all[i], l_all[i])
            col += t
        m = attention_mask[..., col:] if attention_mask is not None else None
        _, _, new = self._decode_multi_eager(query_states, key_states, value_states, past, m, o_all[-1], l_all[-1])
        out = torch.empty((bsz, H, n_q, D), dtype=torch.float16, device=dev)
        lse = torch.empty((bsz, H, n_q), dtype=torch.float32, device=dev) if return_lse else None
        rows = bsz * H * n_q
        with torch.cuda.device(dev):
            err = _lib.load().mustafar_merge_attention_states(torch.cuda.current_stream(dev).cuda_stream, o_all.data_ptr(), rows * D,
                                                              l_all.data_ptr(), rows, parts, rows, D, out.data_ptr(),
                                                              lse.data_ptr() if return_lse else None)
        _lib.check(err, "mustafar_merge_attention_states")
        return (out, lse, new) if return_lse else (out, new)

    # ---- head_dim 64 over a cache that grows by extents (MustafarConfig(hd64_extents=True); cache64.py) ---------------------------------
    def _run_triggers_ext64(self, pasts):
        """The trigger of every layer that is due.  A cache that is still empty (C = 0) gets its base from the window rows the
        reference's way (prune, two-pass conversion: the base is reference-layout arrays); every other layer's 256 rows become an
        extent, all layers in one batched call (ExtentCache64.append_extents).  A full table is consolidated first."""
        kth_k, kth_v = self._kth(self.head_dim)
        out = [Past(*p) for p in pasts]
        groups = {}
        for i, p in enumerate(out):
            if not self.trigger_due(p):
                continue
            k_c, k_w, v_c, v_w = p[:4]
            Bkv = k_w.buf.shape[0] * k_w.buf.shape[1]
            if p.compressed_length == 0:
                k_new, v_new = self._compress_front(k_w.buf, v_w.buf)
                k_c, v_c = self.EXTENT_CACHE_64(k_new, "key", Bkv, 256), self.EXTENT_CACHE_64(v_new, "value", Bkv, 256)
                k_w.drop_front(256)
                v_w.drop_front(256)
                out[i] = p._replace(k_cache=k_c, v_cache=v_c, compressed_length=256)
                continue
            if len(k_c.extents) >= k_c.MAX_EXTENTS:   # table full: one copy of the cache (new addresses), then extents again
                out[i] = p._replace(k_cache=k_c.consolidate(), v_cache=v_c.consolidate())
            groups.setdefault((k_w.len, tuple(k_w.buf.shape)), []).append(i)
        for (wl, _), idxs in groups.items():   # (one group in a model: every layer's window has the same shape and length)
            ExtentCache64.append_extents([(out[i].k_cache, out[i].v_cache) for i in idxs],
                                         [(out[i].k_window.buf, out[i].v_window.buf) for i in idxs], kth_k, kth_v, wl)
            for i in idxs:
                out[i].k_window.len = out[i].v_window.len = wl - 256
                out[i] = out[i]._replace(compressed_length=out[i].compressed_length + 256)
        return out

    # ---- the 256-token trigger of all layers at once (round 4) ----------------------------------------------------------------------
    def trigger_due(self, past) -> bool:
        """The step that produced `past` (its kv_seq_len already counted) reached the trigger of model :324."""
        _, k_w, _, _, C, L = past
        return isinstance(k_w, Window) and (L - self.cfg.residual_length - C) % 256 == 0 and k_w.len >= 256

    def _batched_ok(self, past) -> bool:
        k_c, C = past.k_cache, past.compressed_length
        return self.cfg.extents and isinstance(k_c, CompressedArena) and C > 0 and k_c.tokens % 256 == 0 and \
            len(k_c.extents) < k_c.MAX_EXTENTS and self._reads_extents(C + 256 + past.k_window.cap)

    def prepare_triggers(self, pasts):
        """Allocate and initialise the storage of the coming trigger of every layer ahead of it (one allocation, three launches):
        run_triggers() then allocates nothing.  Returns the pool to hand to run_triggers (None where the batched form does not apply)."""
        pasts = [Past(*p) for p in pasts]
        if not pasts or not all(self._batched_ok(p) for p in pasts):
            return None
        return CompressedArena.prepare_extents([(p.k_cache, p.v_cache) for p in pasts], *self._kth(self.head_dim))

    def run_triggers(self, pasts, pool=None):
        """The trigger (model :324-398) of every layer whose last step reached it (decode_fused(defer_trigger=True), or a replayed
        graph of the step accounted with advance()): prune + compress the 256 oldest window rows of K and V into an extent of the
        cache, slide the windows.  All layers in two library calls and one host read (cache.py: append_extent_pairs) where the cache
        grows by extents; layer by layer otherwise.  Returns the new list of pasts."""
        cfg = self.cfg
        if cfg.hd64_extents:
            return self._run_triggers_ext64(pasts)
        kth_k, kth_v = self._kth(self.head_dim)
        out = [Past(*p) for p in pasts]
        due = [i for i, p in enumerate(out) if self.trigger_due(p)]
        if not due:
            return out
        for i in due:
            if not (isinstance(out[i].k_cache, CompressedArena) or (cfg.arena and out[i].compressed_length == 0)):
                raise RuntimeError("run_triggers works on arena caches (MustafarConfig(arena=True)); a tuple cache runs its trigger inside decode()")
        batch = [i for i in due if self._batched_ok(out[i])]
        wl = {out[i].k_window.len for i in batch}
        if batch and len(wl) == 1 and len({out[i].k_window.buf.shape for i in batch}) == 1:
            CompressedArena.append_extent_pairs([(out[i].k_cache, out[i].v_cache) for i in batch],
                                                [(out[i].k_window.buf, out[i].v_window.buf) for i in batch],
                                                kth_k, kth_v, wl.pop(), pool if len(batch) == len(out) else None)
            for i in batch:
                out[i].k_window.len = out[i].v_window.len = out[i].k_window.len - 256
                out[i] = out[i]._replace(compressed_length=out[i].compressed_length + 256)
        else:
            batch = []
        for i in due:
            if i not in batch:
                out[i] = self._trigger_one(out[i], kth_k, kth_v)
        return out

    def _trigger_one(self, past, kth_k, kth_v):
        """One layer's trigger over an arena cache (the body decode_fused runs when it is not deferred)."""
        cfg = self.cfg
        k_c, k_w, v_c, v_w, C = past[:5]
        if C == 0:
            k_c, v_c = CompressedArena.from_raw_pair(k_w.buf, v_w.buf, 256, kth_k, kth_v, None, self._slack())
            if cfg.extents:
                k_c.ext_table, v_c.ext_table
        elif cfg.extents and k_c.tokens % 256 == 0 and self._reads_extents(C + max(k_w.cap, v_w.cap)):
            if len(k_c.extents) >= k_c.MAX_EXTENTS:          # table full: one copy of the cache, then extents again
                k_c, v_c = k_c.consolidate(), v_c.consolidate()
                k_c.ext_table, v_c.ext_table
            CompressedArena.append_extent_pair(k_c, v_c, k_w.buf, v_w.buf, kth_k, kth_v)
        else:
            if k_c.extents:
                k_c, v_c = k_c.consolidate(), v_c.consolidate()
            CompressedArena.append_window_pair(k_c, v_c, k_w.buf, v_w.buf, 256, kth_k, kth_v)
        Window.drop_front_pair(k_w, v_w, 256)                                                   # :392-393, in place
        return past._replace(k_cache=k_c, v_cache=v_c, compressed_length=C + 256)

    # ---- decode (model :256-400) -----------------------------------------------------------------------------
    def decode(self, query_states, key_states, value_states, past, attention_mask=None):
        """q [B,Hq,1,D], new k/v [B,Hkv,1,D] -> (attn_output [B,Hq,1,D], past)."""
        cfg = self.cfg
        if cfg.api == "fused":
            return self.decode_fused(query_states, key_states, value_states, past, attention_mask=attention_mask)
        past = Past(*past)
        if isinstance(past.k_window, Window):   # a fused cache handed to the unfused path
            past = past._replace(k_window=past.k_window.view(), v_window=past.v_window.view())
        if hasattr(past.k_cache, "to_reference"):   # an arena or an extent cache
            past = past._replace(k_cache=past.k_cache.to_reference(), v_cache=past.v_cache.to_reference())
        bsz, _, q_len, D = query_states.shape
        total_batch_size = bsz * self.num_heads
        total_batch_kv = bsz * self.num_key_value_heads
        groups = self.num_key_value_groups
        k_compressed, k_local_window, v_compressed, v_local_window, compressed_length, _ = past
        kv_seq_len = past.kv_seq_len + 1                                                               # :251
        reference_api = cfg.api == "reference"

        k_local_window = torch.cat([k_local_window, key_states], dim=2)                                # :270
        if compressed_length != 0:
            if reference_api:
                padded_query = F.pad(query_states.view(total_batch_size, -1, D), (0, 0, 0, 7), mode="constant", value=0)   # :273
                att_compressed = _operator_module().mustafar_key_formulation(
                    k_compressed[0], torch.cat(k_compressed[2]), k_compressed[1], k_compressed[3], padded_query,
                    compressed_length, D, total_batch_size, groups)                                    # :274
                att_compressed = att_compressed[:, 0:1, :].view(bsz, self.num_heads, 1, compressed_length)   # :275
            else:
                att_compressed = _operator_module().mustafar_key_formulation(
                    k_compressed[0], k_compressed[2].flat, k_compressed[1], k_compressed[3],
                    query_states.reshape(total_batch_size, 1, D), compressed_length, D, total_batch_size, groups
                ).view(bsz, self.num_heads, 1, compressed_length)
            att_local = torch.matmul(query_states, repeat_kv(k_local_window, groups).transpose(2, 3))  # :278
            att_qkfull = torch.cat([att_compressed, att_local], dim=-1)                                # :279
        else:
            att_qkfull = torch.matmul(query_states, repeat_kv(k_local_window, groups).transpose(2, 3))  # :282
        attn_weights = att_qkfull / math.sqrt(D)                                                       # :284
        if attn_weights.size() != (bsz, self.num_heads, q_len, kv_seq_len):
            raise ValueError(f"Attention weights should be of size {(bsz, self.num_heads, q_len, kv_seq_len)}, "
                             f"but is {attn_weights.size()}")                                          # :287-291
        if attention_mask is not None:                                                                 # :293-301
            attn_weights = attn_weights + attention_mask
            attn_weights = torch.max(attn_weights, torch.tensor(torch.finfo(attn_weights.dtype).min))
        attn_weights = F.softmax(attn_weights, dim=-1, dtype=torch.float32).to(query_states.dtype)     # :304

        v_local_window = torch.cat([v_local_window, value_states], dim=2)                              # :309
        if compressed_length != 0:
            if reference_api:
                padded_score = F.pad(attn_weights[:, :, :, :compressed_length].view(total_batch_size, -1, compressed_length),
                                     (0, 0, 0, 7)).contiguous()                                        # :313
                out_c = _operator_module().mustafar_value_formulation(
                    v_compressed[0], torch.cat(v_compressed[2]), v_compressed[1], v_compressed[3], padded_score,
                    self._ws(query_states.device), D, compressed_length, total_batch_size, groups)     # :314
                out_c = out_c[:, 0:1, :].view(bsz, self.num_heads, 1, D)                               # :315
            else:
                score = attn_weights[:, :, :, :compressed_length].reshape(total_batch_size, 1, compressed_length)
                out_c = _operator_module().mustafar_value_formulation(
                    v_compressed[0], v_compressed[2].flat, v_compressed[1], v_compressed[3], score,
                    self._ws(query_states.device), D, compressed_length, total_batch_size, groups
                ).view(bsz, self.num_heads, 1, D)
            out_l = torch.matmul(attn_weights[:, :, :, compressed_length:], repeat_kv(v_local_window, groups))   # :316
            attn_output = out_c + out_l                                                                # :317
        else:
            attn_output = torch.matmul(attn_weights, repeat_kv(v_local_window, groups))                # :320

        # :324 (the reference would hand a <256-token window to the compressor when this fires with a short
        # window, which asserts there; guard instead)
        if (kv_seq_len - cfg.residual_length - compressed_length) % 256 == 0 and k_local_window.shape[2] >= 256:
            k_new, v_new = self._compress_front(k_local_window, v_local_window)                        # :325-326
            if compressed_length == 0:                                                                 # :327-337
                k_compressed, v_compressed = k_new, v_new
            else:                                                                                      # :339-390
                k_compressed = append_compressed(k_compressed, k_new, total_batch_kv, compressed_length, 256, D)
                v_compressed = append_compressed(v_compressed, v_new, total_batch_kv, compressed_length, 256, D)
            k_local_window = k_local_window[:, :, 256:, :].clone().contiguous()                        # :392
            v_local_window = v_local_window[:, :, 256:, :].clone().contiguous()                        # :393
            compressed_length = compressed_length + 256                                                # :398

        return attn_output, Past(k_compressed, k_local_window, v_compressed, v_local_window, compressed_length, kv_seq_len)

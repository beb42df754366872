"""A dense stand-in for MustafarAttention (a plain module of the suite, not a conftest): the public methods the session executor calls,
over dense rows in plain torch, written from the docstrings of mustafar_amd/hook.py.  The compressed cache is the oracle-pruned rows, the
arithmetic is the hook's in float64 (fp16 scores, fp16 x = score / sqrt(d), the additive mask in fp16 clamped at finfo.min, softmax), a
split call merges the normalised parts by their log-sum-exp.  It runs the executor and its truth bookkeeping on the CPU, and with
`defect=` it is the harness's mutant: each defect below must be caught by the check tests/test_session_plan_host.py names."""
import math
from collections import namedtuple

import torch

from tests.hd64_util import oracle_prune

NEG = torch.finfo(torch.float16).min
Past = namedtuple("Past", "k_cache k_window v_cache v_window compressed_length kv_seq_len")

DEFECTS = (
    "rejected_visible",            # a rejected row stays visible to the next call
    "keep_skips_v",                # keep= gathers K but not V
    "trigger_late",                # the trigger fires one row late
    "trigger_255",                 # the trigger compresses 255 rows
    "split_mask_left",             # the live part of a split call reads its mask columns one to the left
    "hole_unmasked_compressed",    # a hole is unmasked once it is compressed
    "chunk_mask_rows",             # the second chunk of a chunked multi gets the first chunk's mask rows
    "skip_layer",                  # one layer is skipped in run_triggers
)


class FakeWindow:
    def __init__(self, rows, cap):
        Bq, H, w, D = rows.shape
        self.buf = torch.zeros((Bq, H, max(cap, w), D), dtype=rows.dtype, device=rows.device)
        self.buf[:, :, :w] = rows
        self.len = w
        self.stale = 0      # rows behind `len` that the last accept() rejected

    @property
    def cap(self):
        return self.buf.shape[2]

    def view(self):
        return self.buf[:, :, :self.len]

    def append(self, rows):
        n = rows.shape[2]
        if self.len + n > self.cap:
            nb = torch.zeros((*self.buf.shape[:2], self.len + n, self.buf.shape[3]), dtype=self.buf.dtype, device=self.buf.device)
            nb[:, :, :self.len] = self.view()
            self.buf = nb
        self.buf[:, :, self.len:self.len + n] = rows
        self.len += n


class DenseCache:
    """The compressed cache as the dense pruned rows [B, Hkv, tokens, D]."""

    def __init__(self, rows):
        self.rows = rows

    def to_reference(self):
        e = torch.zeros(0, dtype=torch.int16)
        return [self.rows.contiguous().view(torch.int16).reshape(-1), e, e, e]


class FakeShared:
    """One copy of a frozen segment for the whole batch: pruned rows [1, Hkv, tokens, D]."""

    def __init__(self, Kp, Vp):
        self.K, self.V, self.tokens = Kp, Vp, Kp.shape[2]


def make_shared(Kp, Vp):
    return FakeShared(Kp, Vp)


def make_segment(Kp, Vp):
    return DenseCache(Kp), DenseCache(Vp), Kp.shape[2]


def _part(q, K, V, groups, mask=None, new_from=None):
    """Attention of q [B, Hq, n, D] over K / V [B or 1, Hkv, T, D] -> (out float64 [B, Hq, n, D], lse float64 [B, Hq, n]).  mask: additive
    fp16 [B, 1, 1 or n, T].  new_from: the column of the first new row: token j sees the columns below new_from + j + 1."""
    Bq, Hq, n, D = q.shape
    Hkv, T = K.shape[1], K.shape[2]
    K, V = K.expand(Bq, -1, -1, -1), V.expand(Bq, -1, -1, -1)
    qd = q.double().reshape(Bq, Hkv, groups * n, D)
    s = torch.einsum("bkrd,bktd->bkrt", qd, K.double()).half().double()
    x = (s / math.sqrt(D)).half().reshape(Bq, Hq, n, T)
    if mask is not None:
        x = torch.clamp(x + mask.to(torch.float16), min=NEG)
    x = x.double()
    if new_from is not None:
        cols = torch.arange(T, device=q.device)[None, :]
        hidden = cols > new_from + torch.arange(n, device=q.device)[:, None]
        x = x.masked_fill(hidden[None, None], float("-inf"))
    m = x.amax(-1, keepdim=True)
    e = torch.exp(x - m)
    l = e.sum(-1, keepdim=True)
    p = (e / l).reshape(Bq, Hkv, groups * n, T)
    out = torch.einsum("bkrt,bktd->bkrd", p, V.double()).reshape(Bq, Hq, n, D)
    return out, (m + torch.log(l)).squeeze(-1)


def _merge(parts):
    """Normalised parts over disjoint token sets, by their log-sum-exp."""
    lses = torch.stack([l for _, l in parts])
    M = lses.amax(0)
    w = torch.exp(lses - M)
    out = sum(w[i][..., None] * parts[i][0] for i in range(len(parts))) / w.sum(0)[..., None]
    return out, M + torch.log(w.sum(0))


class FakeAttention:
    def __init__(self, num_attention_heads, num_key_value_heads, head_dim, k_sparsity=0.7, v_sparsity=0.7, residual_length=32, defect=None):
        assert defect is None or defect in DEFECTS
        self.num_heads, self.num_key_value_heads, self.head_dim = num_attention_heads, num_key_value_heads, head_dim
        self.groups = num_attention_heads // num_key_value_heads
        self.ks, self.vs, self.R, self.defect = k_sparsity, v_sparsity, residual_length, defect

    # ---- prefill ---------------------------------------------------------------------------------------------------------------------
    def build_cache(self, key_states, value_states):
        """k / v [B, Hkv, L, D] -> past: the first ((L - R) // 256) * 256 rows pruned and compressed, the rest the window."""
        L = key_states.shape[2]
        C = max(0, (L - self.R) // 256 * 256)
        if C == 0:
            return Past(None, key_states, None, value_states, 0, L)
        return Past(DenseCache(oracle_prune(key_states[:, :, :C], self.ks)), key_states[:, :, C:].clone(),
                    DenseCache(oracle_prune(value_states[:, :, :C], self.vs)), value_states[:, :, C:].clone(), C, L)

    def to_fused(self, past):
        k_c, k_w, v_c, v_w, C, L = past
        if not isinstance(k_w, FakeWindow):
            k_w, v_w = FakeWindow(k_w, self.R + 256), FakeWindow(v_w, self.R + 256)
        return Past(k_c, k_w, v_c, v_w, C, L)

    # ---- the trigger ------------------------------------------------------------------------------------------------------------------
    def trigger_due(self, past):
        _, k_w, _, _, C, L = past
        if self.defect == "trigger_late":
            return isinstance(k_w, FakeWindow) and (L - 1 - self.R - C) % 256 == 0 and k_w.len >= 257
        return isinstance(k_w, FakeWindow) and (L - self.R - C) % 256 == 0 and k_w.len >= 256

    def fits_before_trigger(self, past, n_q):
        _, k_w, _, _, C, L = past
        for j in range(n_q - 1):
            if (L + j + 1 - self.R - C) % 256 == 0 and k_w.len + j + 1 >= 256:
                return j + 1
        return n_q

    def _trigger(self, past):
        """Prune and compress the 256 oldest window rows, slide the windows."""
        k_c, k_w, v_c, v_w, C, L = past
        n = 255 if self.defect == "trigger_255" else 256
        new = []
        for w, c, sp_ in ((k_w, k_c, self.ks), (v_w, v_c, self.vs)):
            block = w.buf[:, :, :256].clone()
            block[:, :, :n] = oracle_prune(block[:, :, :n], sp_)
            new.append(DenseCache(block if c is None else torch.cat([c.rows, block], 2)))
            keep = w.buf[:, :, 256:w.len].clone()
            w.len -= 256
            w.buf[:, :, :w.len] = keep
        return Past(new[0], k_w, new[1], v_w, C + 256, L)

    def _close(self, past, defer_trigger):
        if defer_trigger or not self.trigger_due(past):
            return past
        return self._trigger(past)

    def prepare_triggers(self, pasts):
        """Storage of the coming trigger ahead of it: nothing to allocate over dense rows."""
        return None

    def run_triggers(self, pasts, pool=None):
        out = [Past(*p) for p in pasts]
        for i, p in enumerate(out):
            if self.defect == "skip_layer" and i == len(out) - 1 and i > 0:
                continue
            if self.trigger_due(p):
                out[i] = self._trigger(p)
        return out

    # ---- the live call ----------------------------------------------------------------------------------------------------------------
    def _live(self, q, k_rows, v_rows, past, mask, per=None):
        """n new tokens over the live cache: rows appended, nothing compressed -> (out float64, lse float64, past')."""
        past = self.to_fused(past)
        k_c, k_w, v_c, v_w, C, L = past
        n = q.shape[2]
        if mask is not None:
            assert mask.dim() == 4 and mask.shape[2] in (1, n) and mask.shape[3] == L + n, f"mask {tuple(mask.shape)} for {L} + {n} rows"
            if self.defect == "hole_unmasked_compressed" and C:
                mask = mask.clone()
                front = mask[..., :C]
                front[front == NEG] = 0.0
        extra = None
        if k_w.stale and self.defect == "rejected_visible":
            extra = (k_w.buf[:, :, k_w.len:k_w.len + k_w.stale].clone(), v_w.buf[:, :, v_w.len:v_w.len + v_w.stale].clone())
        k_w.stale = v_w.stale = 0
        k_w.append(k_rows)
        v_w.append(v_rows)
        K = k_w.view() if k_c is None else torch.cat([k_c.rows, k_w.view()], 2)
        V = v_w.view() if v_c is None else torch.cat([v_c.rows, v_w.view()], 2)
        per = per or n
        outs, lses = [], []
        for s0 in range(0, n, per):      # more than 64 // groups tokens run as consecutive calls of at most that many
            s1 = min(n, s0 + per)
            m = None
            if mask is not None:
                r0, r1 = (s0, s1) if mask.shape[2] > 1 else (0, 1)
                if self.defect == "chunk_mask_rows" and mask.shape[2] > 1 and s0:
                    r0, r1 = 0, s1 - s0
                m = mask[:, :, r0:r1, :L + s1]
            parts = [_part(q[:, :, s0:s1], K[:, :, :L + s1], V[:, :, :L + s1], self.groups, m, new_from=L + s0)]
            if extra is not None:
                parts.append(_part(q[:, :, s0:s1], extra[0], extra[1], self.groups))
            o, l = _merge(parts) if len(parts) > 1 else parts[0]
            outs.append(o)
            lses.append(l)
        return torch.cat(outs, 2), torch.cat(lses, 2), Past(k_c, k_w, v_c, v_w, C, L + n)

    def decode_fused(self, query_states, key_states, value_states, past, attention_mask=None, defer_trigger=False, return_lse=False):
        """One token: (out [B, H, 1, D], past) or (out, lse fp32 [B, H], past); the trigger runs when it is due unless deferred."""
        assert query_states.shape[2] == 1
        out, lse, new = self._live(query_states, key_states, value_states, past, attention_mask)
        new = self._close(new, defer_trigger)
        return (out.half(), lse[..., 0].float(), new) if return_lse else (out.half(), new)

    def decode_multi(self, query_states, key_states, value_states, past, return_lse=False, attention_mask=None):
        """n_q consecutive tokens; appends and never compresses: accept() closes it."""
        n = query_states.shape[2]
        fits = self.fits_before_trigger(self.to_fused(past), n)
        if fits < n:
            raise ValueError(f"decode_multi: {n} tokens would step over a 256-token trigger point; at most {fits} fit in this call")
        out, lse, new = self._live(query_states, key_states, value_states, past, attention_mask, per=64 // self.groups)
        return (out.half(), lse.float(), new) if return_lse else (out.half(), new)

    def accept(self, past, rejected=0, defer_trigger=False, keep=None, n_q=None):
        past = Past(*past)
        k_w, v_w = past.k_window, past.v_window
        if keep is not None:
            if rejected != 0 or n_q is None:
                raise ValueError("accept: keep= needs n_q and does not go with rejected")
            n_keep, base = keep.shape[1], k_w.len - n_q
            for w in (k_w,) if self.defect == "keep_skips_v" else (k_w, v_w):
                rows = w.buf[:, :, base:base + n_q].clone()
                for b in range(rows.shape[0]):
                    w.buf[b, :, base:base + n_keep] = rows[b][:, keep[b].long().clamp(0, n_q - 1)]
            rejected = n_q - n_keep
        if not 0 <= rejected < k_w.len:
            raise ValueError(f"accept: rejected must be in [0, {k_w.len})")
        k_w.len -= rejected
        v_w.len -= rejected
        k_w.stale = v_w.stale = rejected
        return self._close(past._replace(kv_seq_len=past.kv_seq_len - rejected), defer_trigger)

    # ---- frozen segments --------------------------------------------------------------------------------------------------------------
    def decode_segment_multi(self, query_states, k_cache, v_cache=None, tokens=None, attention_mask=None):
        """n_q tokens over ONE frozen segment, every token sees all of it -> (out fp16, lse fp32 [B, H, n_q])."""
        out, lse = self._segment(query_states, k_cache if v_cache is None else (k_cache, v_cache, tokens), attention_mask)
        return out.half(), lse.float()

    def _segment(self, q, f, mask):
        if isinstance(f, FakeShared):
            if mask is not None:
                raise ValueError("a shared segment takes no attention mask")
            return _part(q, f.K, f.V, self.groups)
        return _part(q, f[0].rows, f[1].rows, self.groups, mask)

    def _split(self, q, k_rows, v_rows, past, frozen, mask, per=None):
        past = Past(*past)
        n = q.shape[2]
        tokens = [f.tokens if isinstance(f, FakeShared) else int(f[2]) for f in frozen]
        if mask is not None:
            assert mask.shape[3] == sum(tokens) + past.kv_seq_len + n
        parts, col = [], 0
        for f, t in zip(frozen, tokens):      # a shared entry's columns are skipped, a per-sequence entry reads its own
            shared = isinstance(f, FakeShared)
            parts.append(self._segment(q, f, None if mask is None or shared else mask[..., col:col + t]))
            col += t
        m = None
        if mask is not None:
            m = mask[..., col - 1:-1] if self.defect == "split_mask_left" and col else mask[..., col:]
        o, l, new = self._live(q, k_rows, v_rows, past, m, per)
        out, lse = _merge(parts + [(o, l)])
        return out, lse, new

    def decode_split(self, query_states, key_states, value_states, past, frozen, attention_mask=None):
        """One step over frozen segments + the live cache; no mask next to a shared entry; the trigger runs on the live cache."""
        if attention_mask is not None and any(isinstance(f, FakeShared) for f in frozen):
            raise ValueError("decode_split: a SharedSegment in `frozen` takes no attention mask")
        out, _, new = self._split(query_states, key_states, value_states, past, list(frozen), attention_mask)
        return out.half(), self._close(new, False)

    def decode_multi_split(self, query_states, key_states, value_states, past, frozen, attention_mask=None, return_lse=False):
        n = query_states.shape[2]
        fits = self.fits_before_trigger(self.to_fused(past), n)
        if fits < n:
            raise ValueError(f"decode_multi_split: {n} tokens would step over a 256-token trigger point; at most {fits} fit in this call")
        out, lse, new = self._split(query_states, key_states, value_states, past, list(frozen), attention_mask, per=64 // self.groups)
        return (out.half(), lse.float(), new) if return_lse else (out.half(), new)

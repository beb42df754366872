"""Executor of the long decode sessions (a plain module of the suite, not a conftest): runs a plan of tests/session_plan.py on an attention
object -- MustafarAttention on the GPU, the dense stand-in of tests/session_fake.py on the CPU -- against the truth it keeps itself.

The truth is the dense rows K, V [layers, B, Hkv, L, D] as the cache should hold them: every row that stayed (holes included) in order, the
first C of them pruned by the oracle's rule (partial_util.pruned_rows), and a hole mask per sequence.  Rows a sequence rejects, holes and
left padding carry poison -- K rows at four times the normal scale, V rows of constant 8 --, so a leak moves the output far outside the
bound.

After every op the hook's compressed_length, kv_seq_len and both Window.len are held against the planner's.  After every decode op, for
every query token j: |out - exact_data.hook_model| / bound <= 1 over the rows token j sees (a split call: shared_util.split_bound over its
parts, as tests/test_gpu_multi_split.py does), and the same for an LSE with partial_util.lse_model; outputs are checked finite.  After every
trigger and at the end a twin to_fused(build_cache(truth rows)) must hold the same compressed cache and windows bit for bit.  No tolerance
of its own.  Every op of the plan is run; a check that fails raises SessionFailure naming the check."""
from collections import Counter

import torch

from tests import exact_data as xd
from tests import multi_split_util as mu
from tests import partial_util as pu
from tests import session_plan as sp
from tests import shared_util as su
from tests.multi_split_util import bits

NEG = torch.finfo(torch.float16).min
POISON_K, POISON_V = 4.0, 8.0


class SessionFailure(AssertionError):
    """check: lengths | finite | ratio | lse | twin_cache | twin_window | negative_control."""

    def __init__(self, check, index, op, msg):
        super().__init__(f"op {index} {op}: [{check}] {msg}")
        self.check, self.index, self.op = check, index, op


def _reference(c):
    c = c.to_reference() if hasattr(c, "to_reference") else c
    nz = c[2]
    return [c[0].reshape(-1), c[1].reshape(-1), nz if isinstance(nz, torch.Tensor) else torch.cat(list(nz)), c[3].reshape(-1)]


def same_cache(a, b):
    """tests/test_gpu_multi_query._same_cache: the reference layout of both, array by array."""
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(_reference(a), _reference(b)))


class Session:
    def __init__(self, kind, seed, attn, device, make_shared=None, make_segment=None, choice=None, plan=None):
        """attn: the attention object; make_shared(Kp [1, Hkv, t, D], Vp) / make_segment(Kp [B, Hkv, t, D], Vp): the frozen entries of the
        kind's cache kind from pruned rows (tests/test_gpu_shared_segment._shared_of, tests/test_gpu_partial._segment_cache); choice: what
        reports the kernel the last call launched (mustafar_last_decode_choice), or None; plan: the ops to run instead of plan(kind, seed)."""
        self.kind, self.seed, self.k = kind, seed, sp.KINDS[kind]
        self.attn, self.dev, self.choice = attn, device, choice
        self.D, self.groups, self.layers = self.k["head_dim"], self.k["groups"], self.k["layers"]
        self.Hq = sp.HKV * self.groups
        self.gen = torch.Generator().manual_seed(1000 * sorted(sp.KINDS).index(kind) + seed)
        self.worst, self.choices, self.control = Counter(), Counter(), None
        h = sp.header(kind, seed)
        self.plan = sp.plan(kind, seed) if plan is None else plan      # (plan: a reduced op list of a regression case)
        Lmax = max(op["L"] for op in self.plan) + 8
        L0, pad = h["start"], h["pad"]
        self.hole = torch.zeros((sp.B, Lmax), dtype=torch.bool)
        self.hole[1, :pad] = True
        self.K = torch.zeros((self.layers, sp.B, sp.HKV, Lmax, self.D), dtype=torch.float16, device=device)
        self.V = torch.zeros_like(self.K)
        k0, v0 = self._rows(L0, [[], list(range(pad))])
        self.K[:, :, :, :L0], self.V[:, :, :, :L0] = k0, v0
        self.L = L0
        self.C = max(0, (L0 - sp.R) // sp.BLOCK * sp.BLOCK)
        self.Kp, self.Vp = self.K.clone(), self.V.clone()
        self._prune()
        self.pasts = [attn.to_fused(attn.build_cache(self.K[l, :, :, :L0].contiguous(), self.V[l, :, :, :L0].contiguous()))
                      for l in range(self.layers)]
        self.frozen = {}
        if self.k["split"]:
            ks, vs = self.k["k_sparsity"], self.k["v_sparsity"]
            Ks, Vs = pu.pruned_rows(self._randn((1, sp.HKV, sp.F_SHARED, self.D)), self._randn((1, sp.HKV, sp.F_SHARED, self.D)), sp.F_SHARED, ks, vs)
            Kq, Vq = pu.pruned_rows(self._randn((sp.B, sp.HKV, sp.F_SEQ, self.D)), self._randn((sp.B, sp.HKV, sp.F_SEQ, self.D)), sp.F_SEQ, ks, vs)
            self.frozen = {"s": (make_shared(Ks, Vs), Ks.expand(sp.B, -1, -1, -1), Vs.expand(sp.B, -1, -1, -1), sp.F_SHARED),
                           "p": (make_segment(Kq, Vq), Kq, Vq, sp.F_SEQ)}
        self.first0 = None      # kv_seq_len before the several-token call that is still open

    # ---- data ---------------------------------------------------------------------------------------------------------------------
    def _randn(self, shape):
        return torch.randn(shape, generator=self.gen).half().to(self.dev)

    def _rows(self, n, poison):
        """New K / V rows [layers, B, Hkv, n, D]; poison[b]: the rows of sequence b that carry poison."""
        k, v = self._randn((self.layers, sp.B, sp.HKV, n, self.D)), self._randn((self.layers, sp.B, sp.HKV, n, self.D))
        for b, rows in enumerate(poison):
            if rows:
                k[:, b, :, rows] = k[:, b, :, rows] * POISON_K
                v[:, b, :, rows] = POISON_V
        return k, v

    def _prune(self):
        """The first C rows of the truth as the cache holds them."""
        if self.C:
            for l in range(self.layers):
                kp, vp = pu.pruned_rows(self.K[l, :, :, :self.C], self.V[l, :, :, :self.C], self.C, self.k["k_sparsity"], self.k["v_sparsity"])
                self.Kp[l, :, :, :self.C], self.Vp[l, :, :, :self.C] = kp, vp

    # ---- masks --------------------------------------------------------------------------------------------------------------------
    def _mask(self, op, n, frozen):
        """(mask handed to the call, mask of the model, the model's mask with the holes unmasked) [B, 1, 1 or n, frozen + L + n] or Nones.
        The columns of a shared entry hold finfo.min in the call's mask -- nobody reads them -- and 0 in the model's."""
        kind = op.get("mask", "none")
        holes = bool(self.hole[:, :self.L].any())
        if kind == "none" and not holes:
            return None, None, None
        Fc = sum(self.frozen[f][3] for f in frozen)
        first, total = self.L, Fc + self.L + n
        rows = n if kind in ("causal", "tree") else 1
        m = torch.zeros((sp.B, 1, rows, total), dtype=torch.float16)
        if kind == "row":     # finite values that are fp16 numbers, on every column a call reads
            m += torch.randint(-8, 1, m.shape, generator=self.gen).half() * 0.25
        for j in range(rows if kind in ("causal", "tree") else 0):
            if kind == "causal":
                m[:, :, j, Fc + first + j + 1:] = NEG
            else:
                m[:, :, j, Fc + first:] = NEG
                node = j
                while node >= 0:
                    m[:, :, j, Fc + first + node] = 0.0
                    node = op["parents"][node]
        open_ = m.clone()
        for b in range(sp.B):
            m[b, :, :, Fc:Fc + self.L][..., self.hole[b, :self.L]] = NEG
        call = m.clone()
        if "s" in frozen:
            open_[..., :sp.F_SHARED], m[..., :sp.F_SHARED] = 0.0, 0.0
            call[..., :sp.F_SHARED] = NEG
        return call.to(self.dev), m.to(self.dev), (open_.to(self.dev) if holes else None)

    # ---- the models -----------------------------------------------------------------------------------------------------------------
    def _model(self, q, K, V, mask, want_lse=True):
        """The float64 models for tokens q [B, Hq, m, D] that all see the same rows K / V [B, Hkv, T, D] (mask [B, 1, 1 or m, T] or None):
        (out, bound [B, Hq, m, D], lse, bound [B, Hq, m]).  q's memory is [B, Hkv, groups * m, D]: m tokens at `groups` q heads per kv head
        are, row for row, one token at groups * m (tests/multi_split_util.py), so one evaluation serves them all."""
        m = q.shape[2]
        q1 = mu.as_one_token(q)
        mm = None if mask is None else mu.row_mask(mask, sp.HKV, self.groups, m)
        want, bound = xd.hook_model(q1, K, V, self.groups * m, mask=mm)
        shape = (sp.B, self.Hq, m)
        if not want_lse:
            return want.reshape(*shape, self.D), bound.reshape(*shape, self.D), None, None
        lse, lse_bound = pu.lse_model(q1, K, self.groups * m, mask=mm)
        return want.reshape(*shape, self.D), bound.reshape(*shape, self.D), lse.reshape(shape), lse_bound.reshape(shape)

    def _ratios(self, l, out, lse, q, frozen, first, mask, whole_sight):
        """(max |out - model| / bound, the same of the LSE or None) over the query tokens of one call of layer l.  Token j sees the frozen
        rows and live rows [0, first + j + 1); whole_sight (a draft tree): every new row, the mask hides what the tree does."""
        n = q.shape[2]
        cuts = [0]
        for f in frozen:
            cuts.append(cuts[-1] + self.frozen[f][3])
        Fc = cuts[-1]
        fro_k = [self.frozen[f][1] for f in frozen]
        fro_v = [self.frozen[f][2] for f in frozen]
        # every token sees all of a frozen entry: one evaluation per entry
        fro = [self._model(q, kf, vf, None if mask is None else mask[..., a:b]) for kf, vf, a, b in zip(fro_k, fro_v, cuts, cuts[1:])]
        r_out, r_lse = 0.0, (0.0 if lse is not None and not frozen else None)
        lse = None if lse is None else lse.reshape(sp.B, self.Hq, -1)
        for js in ([slice(0, n)] if whole_sight else [slice(j, j + 1) for j in range(n)]):
            Lj = first + js.stop
            qj = q[:, :, js]
            mj = None if mask is None else (mask if mask.shape[2] == 1 else mask[:, :, js])[..., :Fc + Lj]
            Kl, Vl = self.Kp[l, :, :, :Lj], self.Vp[l, :, :, :Lj]
            want, bound, want_l, bound_l = self._model(qj, torch.cat(fro_k + [Kl], 2), torch.cat(fro_v + [Vl], 2), mj) if frozen else \
                self._model(qj, Kl, Vl, mj, want_lse=r_lse is not None)
            if frozen:   # the split bound of DESIGN.md 4.9 over the parts, token by token
                live = self._model(qj, Kl, Vl, None if mj is None else mj[..., Fc:])
                for t in range(js.stop - js.start):
                    parts, lse_bounds = [], []
                    for o_i, _, l_i, bl_i in [tuple(x[:, :, js] for x in f) for f in fro] + [live]:
                        parts.append((o_i[:, :, t:t + 1], torch.exp(l_i[:, :, t] - want_l[:, :, t])))
                        lse_bounds.append(bl_i[:, :, t])
                    bound[:, :, t:t + 1] = su.split_bound(parts, lse_bounds, want[:, :, t:t + 1], bound[:, :, t:t + 1])
            r = (out[:, :, js].double() - want).abs() / bound
            r_out = max(r_out, float(r.max()) if torch.isfinite(r).all() else float("inf"))
            if r_lse is not None:
                r_lse = max(r_lse, pu.lse_ratio(lse[:, :, js], want_l, bound_l))
        return r_out, r_lse

    # ---- ops ------------------------------------------------------------------------------------------------------------------------
    def _fail(self, check, msg):
        raise SessionFailure(check, self.i, {k: v for k, v in self.op.items() if k in ("op", "n_q", "mask", "frozen", "rejected", "L", "C", "W")}, msg)

    def _lengths(self):
        op = self.op
        for l, p in enumerate(self.pasts):
            got = (p[4], p[5], p[1].len, p[3].len)
            if got != (op["C"], op["L"], op["W"], op["W"]):
                self._fail("lengths", f"layer {l}: compressed_length, kv_seq_len, window lengths {got}, planned {(op['C'], op['L'], op['W'], op['W'])}")
            if op["extents"] is not None and hasattr(p[0], "extents") and (len(p[0].extents), len(p[2].extents)) != (op["extents"],) * 2:
                self._fail("lengths", f"layer {l}: {len(p[0].extents)} / {len(p[2].extents)} extents listed, planned {op['extents']}")

    def _decode(self, op):
        name = op["op"]
        n = op.get("n_q", 1)
        frozen = list(op.get("frozen", ""))
        first = self.L
        q = self._randn((self.layers, sp.B, self.Hq, n, self.D))
        k, v = self._rows(n, op.get("poison", [[], []]))
        for X, x in ((self.K, k), (self.V, v), (self.Kp, k), (self.Vp, v)):
            X[:, :, :, first:first + n] = x
        call_mask, mask, open_mask = self._mask(op, n, frozen)
        entries = [self.frozen[f][0] for f in frozen]
        attn = self.attn
        for l in range(self.layers):
            past, lse = self.pasts[l], None
            kw = dict(attention_mask=call_mask)
            if name in ("multi", "multi_split") and attn.fits_before_trigger(past, n) != n:
                self._fail("lengths", f"fits_before_trigger says {attn.fits_before_trigger(past, n)} of {n} tokens fit")
            if name == "step":
                if op.get("defer"):
                    kw["defer_trigger"] = True
                if op["lse"]:
                    out, lse, new = attn.decode_fused(q[l], k[l], v[l], past, return_lse=True, **kw)
                else:
                    out, new = attn.decode_fused(q[l], k[l], v[l], past, **kw)
            elif name == "multi":
                if op["lse"]:
                    out, lse, new = attn.decode_multi(q[l], k[l], v[l], past, return_lse=True, **kw)
                else:
                    out, new = attn.decode_multi(q[l], k[l], v[l], past, **kw)
            elif name == "split":
                out, new = attn.decode_split(q[l], k[l], v[l], past, entries, **kw)
            else:
                out, lse, new = attn.decode_multi_split(q[l], k[l], v[l], past, entries, return_lse=True, **kw)
            if self.choice is not None:
                self.choices[self.choice()] += 1
            self.pasts[l] = new
            if not torch.isfinite(out.float()).all() or (lse is not None and not torch.isfinite(lse).all()):
                self._fail("finite", f"layer {l}: NaN / Inf in out or lse")
            if name in ("multi", "multi_split") and bool(attn.trigger_due(new)) != op["last_row_is_point"]:
                self._fail("lengths", f"layer {l}: trigger_due is {attn.trigger_due(new)} after the call")
            tree = op.get("mask") == "tree"
            r_out, r_lse = self._ratios(l, out, lse, q[l], frozen, first, mask, tree)
            self.worst[name] = max(self.worst[name], r_out)
            if r_lse is not None:
                self.worst[name + "/lse"] = max(self.worst[name + "/lse"], r_lse)
            if r_out > 1.0:
                self._fail("ratio", f"layer {l}: |out - model| / bound = {r_out:.3f}")
            if r_lse is not None and r_lse > 1.0:
                self._fail("lse", f"layer {l}: |lse - model| / bound = {r_lse:.3f}")
            if open_mask is not None and self.control is None:
                # the negative control: the model with the holes unmasked must NOT fit
                self.control, _ = self._ratios(l, out, None, q[l], frozen, first, open_mask, tree)
                if not self.control > 1.0:
                    self._fail("negative_control", f"the model with the holes unmasked fits ({self.control:.3f}): a leak would not show")
        self.L = first + n
        self.first0 = first

    def _accept(self, op):
        first, n = self.first0, op["n_q"]
        kw = dict(defer_trigger=True) if op.get("defer") else {}
        if op["keep"] is None:
            self.pasts = [self.attn.accept(p, rejected=op["rejected"], **kw) for p in self.pasts]
            self.L -= op["rejected"]
        else:
            keep = torch.tensor(op["keep"], device=self.dev)
            self.pasts = [self.attn.accept(p, keep=keep, n_q=n, **kw) for p in self.pasts]
            n_keep = keep.shape[1]
            for X in (self.K, self.V, self.Kp, self.Vp):
                for b in range(sp.B):
                    X[:, b, :, first:first + n_keep] = X[:, b, :, first:first + n][:, :, keep[b]]
            self.L = first + n_keep
            for b, rows in enumerate(op["new_holes"]):
                self.hole[b, rows] = True

    def _run_triggers(self, op):
        pool = self.attn.prepare_triggers(self.pasts) if op["pool"] else None
        self.pasts = list(self.attn.run_triggers(self.pasts, pool))

    def _twin(self):
        """The cache a prefill of the truth's rows builds: equal bit for bit."""
        for l, p in enumerate(self.pasts):
            t = self.attn.to_fused(self.attn.build_cache(self.K[l, :, :, :self.L].contiguous(), self.V[l, :, :, :self.L].contiguous()))
            if t[4] != p[4] or (p[0] is None) != (t[0] is None):
                self._fail("twin_cache", f"layer {l}: {p[4]} compressed tokens, the twin holds {t[4]}")
            if p[0] is not None and not (same_cache(p[0], t[0]) and same_cache(p[2], t[2])):
                self._fail("twin_cache", f"layer {l}: the compressed cache differs from a prefill of the same rows")
            for i in (1, 3):
                if p[i].len != t[i].len or not torch.equal(bits(p[i].view()), bits(t[i].view())):
                    self._fail("twin_window", f"layer {l}: the {'KV'[i // 2]} window differs from a prefill of the same rows")

    def run(self):
        for self.i, self.op in enumerate(self.plan):
            op = self.op
            {"step": self._decode, "multi": self._decode, "split": self._decode, "multi_split": self._decode, "accept": self._accept,
             "run_triggers": self._run_triggers}[op["op"]](op)
            if op["fired"]:
                self.C += sp.BLOCK
            self._lengths()
            if self.L != op["L"] or self.C != op["C"]:
                self._fail("lengths", f"the truth holds {self.L} rows, {self.C} compressed; planned {op['L']}, {op['C']}")
            if op["fired"]:      # the trigger ran: the truth's first C rows pruned, and a prefill of the same rows as the twin
                self._prune()
                self._twin()
        self._twin()
        return dict(ops=len(self.plan), worst=dict(self.worst), choices=dict(self.choices), control=self.control)


def run_session(kind, seed, attn, device, make_shared=None, make_segment=None, choice=None):
    return Session(kind, seed, attn, device, make_shared, make_segment, choice).run()

"""GPU: long random sessions of the decode API against a dense model -- single steps, several-token calls with masks and draft trees,
accept(rejected=) / accept(keep=), split calls over frozen and shared segments and deferred triggers in turn, over ONE long-lived cache per
layer that goes through four triggers (and, where the extent table is cut to two entries, a consolidation), with masked holes.

The plans come from tests/session_plan.py (conditions: tests/test_session_plan_host.py), the executor and its truth from
tests/session_util.py: lengths after every op, the float64 models with their derived bounds after every decode op for every query token,
a twin prefill bit for bit after every trigger and at the end, one negative control per session.  DESIGN.md 4.15."""
from collections import Counter

import pytest
import torch

from tests import session_plan as sp
from tests import session_util as sx
from tests.hd64_util import DEV

pytestmark = pytest.mark.gpu


def _attention(kind, monkeypatch):
    from mustafar_amd.cache import CompressedArena
    from mustafar_amd.cache64 import ExtentCache64
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    k = sp.KINDS[kind]
    attn = MustafarAttention(MustafarConfig(num_attention_heads=sp.HKV * k["groups"], num_key_value_heads=sp.HKV, head_dim=k["head_dim"],
                                            k_sparsity=k["k_sparsity"], v_sparsity=k["v_sparsity"], api="fused", **k["cfg"]))
    assert attn.cfg.residual_length == sp.R
    if k["small_table"] == "arena":        # as tests/test_gpu_extents.py does: the third extent meets a full table
        monkeypatch.setattr(CompressedArena, "MAX_EXTENTS", 2)
    elif k["small_table"] == "ext64":      # as tests/test_gpu_headdim64_extents.py does
        class Small(ExtentCache64):
            MAX_EXTENTS = 2
        attn.EXTENT_CACHE_64 = Small
    return attn


def _run(kind, seed, monkeypatch, plan=None):
    from mustafar_amd import _lib
    from tests.test_gpu_partial import _segment_cache
    from tests.test_gpu_shared_segment import _shared_of
    attn = _attention(kind, monkeypatch)
    frozen_kind = sp.KINDS[kind]["split"]
    s = sx.Session(kind, seed, attn, DEV, lambda Kp, Vp: _shared_of(frozen_kind, Kp, Vp),
                   lambda Kp, Vp: _segment_cache(frozen_kind, Kp.contiguous(), Vp.contiguous(), attn),
                   choice=_lib.load().mustafar_last_decode_choice, plan=plan)
    return s, s.run()


@pytest.mark.parametrize("kind,seed", sp.SESSIONS)
def test_a_long_session_against_the_dense_model(kind, seed, monkeypatch):
    s, rep = _run(kind, seed, monkeypatch)
    torch.cuda.synchronize()
    calls = Counter(op["op"] for op in s.plan)
    print(f"{kind} seed {seed}: {rep['ops']} ops {dict(calls)}, {s.L} rows, {s.C} compressed")
    print("  worst |kernel - model| / bound per op: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(rep["worst"].items())))
    print("  mustafar_last_decode_choice() after the library calls: " + ", ".join(f"{c:#x} x{n}" for c, n in sorted(rep["choices"].items())))
    print(f"  negative control (the holes unmasked in the model): {rep['control']:.1f}")
    assert all(r <= 1.0 for r in rep["worst"].values()) and rep["control"] > 1.0
    assert s.C == s.plan[-1]["C"] >= 4 * 256 and len(s.plan) == rep["ops"]


# ---- regression cases: the shortest op lists of sessions that failed -------------------------------------------------------------------------
# decode_split over a per-sequence CompressedArena entry of 192 tokens: decode_segment sent every arena to the extents entry point with an
# LSE, which takes a base of whole 256-token blocks -- "HIP error 1 (invalid argument)" on the first split op of every arena session
ARENA_SEGMENT_OF_192 = [dict(op="split", frozen="p", L=301, C=256, W=45, fired=False, holes_compressed=0, full_table=False, extents=None)]


def test_regression_decode_split_over_an_arena_segment_of_192_tokens(monkeypatch):
    s, rep = _run("arena_inplace", 1, monkeypatch, plan=ARENA_SEGMENT_OF_192)
    print(f"decode_split over [a per-sequence arena entry of {sp.F_SEQ} tokens]: |split - whole model| / bound = {rep['worst']['split']:.3f}")
    assert rep["ops"] == 1 and rep["worst"]["split"] <= 1.0 and s.L == 301

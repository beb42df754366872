"""CPU: the runs recorded from the reference's own decode forward (tests/golden/forward_*.npz, written by oracle/gen_golden.py:
`LlamaFlashAttention_MUSTAFAR.forward`, models/llama_mustafar_kernel.py:199-457, executed unchanged) against what this project wrote
itself: the closed form of the trigger rule, the oracle's prune + conversion, exact_data.hook_model and the oracle's SpMV.  The same
recordings hold the hook on the GPU (tests/test_gpu_forward_golden.py).

Worst |recorded output - hook_model| per scenario, in units of hook_model's own bound / of reference_bound (the bound asserted), all
steps: append 0.314 / 0.131, first 0.258 / 0.138, mask 0.496 / 0.220, d64 0.271 / 0.112 (printed by test_recorded_outputs)."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from tests import forward_golden_util as fg
from tests.util import fp16_bound

RAN = ["append", "first", "mask", "d64"]   # scenarios the reference ran to the end


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return {name: fg.load(golden_dir, name) for name in fg.SCENARIOS}


def test_fixture_sizes(golden_dir):
    import os
    for name in fg.SCENARIOS:
        assert os.path.getsize(os.path.join(golden_dir, f"forward_{name}.npz")) <= fg.MAX_FIXTURE_BYTES


@pytest.mark.parametrize("name,compressed,window", [
    ("append", [256] * 6 + [512] * 3, [282, 283, 284, 285, 286, 287, 32, 33, 34]),          # trigger at kv = 544 (step 5)
    ("first", [0] * 6 + [256] * 4, [282, 283, 284, 285, 286, 287, 32, 33, 34, 35]),          # first compression at kv = 288 (step 5)
    ("mask", [256] * 5, [44, 45, 46, 47, 48]),
    ("d64", [256] * 6 + [512] * 3, [282, 283, 284, 285, 286, 287, 32, 33, 34]),
    ("short", [-256], [30]),                                                                # :416 below residual_length: -256, every row in the window
])
def test_recorded_bookkeeping(fixtures, name, compressed, window):
    """compressed_length, the window length and kv_seq_len of every recorded step obey :416 (prefill) and :324 / :398 (decode)."""
    fx = fixtures[name]
    s = fx.spec
    R = fx.recorded_steps
    assert fx["compressed_length"].tolist() == compressed and fx["window_len"].tolist() == window
    assert fx["kv_seq_len"].tolist() == [s["L0"] + i for i in range(R + 1)]
    C = ((s["L0"] - fg.RESIDUAL) // 256) * 256                                              # :416
    assert fx["compressed_length"][0] == C
    for i in range(R):
        kv = s["L0"] + i + 1
        C += 256 if (kv - fg.RESIDUAL - C) % 256 == 0 else 0                                # :324, :398
        assert fx["compressed_length"][i + 1] == C and fx["window_len"][i + 1] == kv - C
    cl, wl, kvs = fg.closed_form(s["L0"], R)
    assert np.array_equal(cl, fx["compressed_length"]) and np.array_equal(wl, fx["window_len"]) and np.array_equal(kvs, fx["kv_seq_len"])
    if name in RAN:
        assert R == s["steps"] and fx.meta["result"] == "ran"
        # snapshots: the prefill, every trigger step, the last step
        trig = [i for i in range(R) if compressed[i + 1] != compressed[i]]
        assert fx["snap_after"].tolist() == [-1] + trig + [R - 1]


def test_short_records_what_the_reference_does(fixtures):
    """A prefill of 30 < residual_length tokens: :416 leaves compressed_length = -256, and the first decode step hands that to the key
    operator (:272-274) -- the reference never reaches its trigger on a 32-row window at kv = 32.  The hook clamps at 0 and guards the
    trigger instead (hook.py: build_cache, decode); tests/test_gpu_forward_golden.py holds that behaviour."""
    fx = fixtures["short"]
    assert fx.recorded_steps == 0
    assert fx.meta["result"] == "OperatorRefused at step 0: mustafar_key_formulation called with compressed_length -256"
    snap = fx.snapshot(-1)
    assert snap["k_win"].shape == (1, 1, 30, 128) and snap["k_bmp"].size == 0 and snap["k_nz"].size == 0


@pytest.mark.parametrize("name", RAN)
def test_recorded_caches(fixtures, name):
    """Every recorded cache equals oracle prune + oracle conversion of the raw rows bit for bit, its nz_offset the oracle's rule (the
    reference's in-place `[1:] += cumsum` of :341-344 included), and both windows hold the raw rows behind the compressed ones."""
    fx = fixtures[name]
    s = fx.spec
    _, K, V, _ = fx.inputs()
    heads = s["bsz"] * s["Hkv"]
    seen = set()
    for after in fx["snap_after"].tolist():
        snap = fx.snapshot(after)
        C, kv = int(fx["compressed_length"][after + 1]), int(fx["kv_seq_len"][after + 1])
        seen.add(C)
        for side, X, sp, conv in (("k", K, fg.K_SPARSITY, orc.convert_key_batched), ("v", V, fg.V_SPARSITY, orc.convert_value_batched)):
            assert np.array_equal(snap[f"{side}_win"], X[:, :, C:kv].numpy().view(np.uint16)), (name, after, side)
            if C == 0:
                assert f"{side}_bmp" not in snap
                continue
            bmp, accum, nzs = conv(orc.prune_magnitude(X[:, :, :C].numpy(), sp).reshape(heads, C, s["D"]))
            assert snap[f"{side}_bmp"].dtype == np.int64 and snap[f"{side}_idx"].dtype == np.int32 and snap[f"{side}_nz_offset"].dtype == np.int32
            assert np.array_equal(snap[f"{side}_bmp"], bmp), (name, after, side)
            assert np.array_equal(snap[f"{side}_idx"], accum), (name, after, side)
            assert np.array_equal(snap[f"{side}_nz"], np.concatenate(nzs).view(np.uint16)), (name, after, side)
            assert np.array_equal(snap[f"{side}_nz_offset"], orc.nz_offset_from_idx(accum)), (name, after, side)
            if name == "append" and side == "k":
                assert len(set(np.diff(snap[f"{side}_nz_offset"]).tolist())) > 1      # a non-trivial cumsum
    assert seen == set(fx["compressed_length"].tolist())


@pytest.mark.parametrize("name", RAN)
def test_recorded_outputs(fixtures, name):
    """Every recorded output lies within reference_bound of hook_model over the oracle-pruned dense K / V -- the masked scenario with its
    finite biases included.  If this bound is ever exceeded the model or the fixture is wrong: find out which; the bound stays."""
    fx = fixtures[name]
    worst_hook = worst_ref = 0.0
    for i in range(fx.recorded_steps):
        m = fg.step_model(fx, i)
        err = (m["rec"].double() - m["model"]).abs()
        assert torch.isfinite(m["rec"]).all()
        r_hook, r_ref = float((err / m["hook_bound"]).max()), float((err / m["ref_bound"]).max())
        print(f"{name} step {i} (C {m['C']}, kv {m['kv']}): |recorded - model| / hook_model bound {r_hook:.3f}, / reference_bound {r_ref:.3f}")
        worst_hook, worst_ref = max(worst_hook, r_hook), max(worst_ref, r_ref)
        assert r_ref <= 1.0, f"{name} step {i}: the recorded output is {r_ref:.3f} x reference_bound away from hook_model"
    print(f"{name}: worst {worst_hook:.3f} of hook_model's bound, {worst_ref:.3f} of reference_bound")
    if name == "mask":   # the mask did something: entry 1 ignores its first 270 columns, entry 0's biased columns moved the output
        m = fg.step_model(fx, 0)
        unmasked, _, _ = fg.reference_bound(m["q"], *fg.dense_kv(*fx.inputs()[1:3], m["C"], m["kv"]), m["C"], 4, None)
        for b in range(2):
            assert float(((unmasked[b] - m["model"][b]).abs() / m["ref_bound"][b]).max()) > 1.0


@pytest.mark.parametrize("name", RAN)
def test_oracle_spmv_matches_logged_sums(fixtures, name):
    """orc.key_spmv / orc.value_spmv over the logged operands of the last step's calls (the 8-row operand, rows 1-7 zero; the cache of the
    last snapshot, addressed through nz_offset) against the float64 sums the generator's numpy stand-ins formed from the same flat arrays."""
    fx = fixtures[name]
    s = fx.spec
    log = {c["name"]: c for c in fx.meta["operator_log"]}
    assert set(log) == {"key", "value"}
    snap = fx.snapshot(fx.recorded_steps - 1)
    T, D, BH, groups = int(fx["compressed_length"][-1]), s["D"], s["bsz"] * s["Hq"], s["Hq"] // s["Hkv"]
    assert log["key"]["scalars"] == [T, D, BH, groups] and log["value"]["scalars"] == [D, T, BH, groups]
    assert log["key"]["shapes"][4] == [BH, 8, D] and log["value"]["shapes"][4] == [BH, 8, T]
    assert log["key"]["dtypes"] == ["torch.int64", "torch.float16", "torch.int32", "torch.int32", "torch.float16"] == log["value"]["dtypes"]
    for which, side, fn, inner, outer in (("key", "k", orc.key_spmv, D, T), ("value", "v", orc.value_spmv, T, D)):
        B = np.zeros((BH, 8, inner), np.float16)
        B[:, 0] = fx[f"log_{which}_b"].view(np.float16)
        C16, C64 = fn(snap[f"{side}_bmp"], snap[f"{side}_nz"].view(np.float16), snap[f"{side}_idx"], snap[f"{side}_nz_offset"], B,
                      outer, inner, BH, groups)
        want, sumabs = fx[f"log_{which}_sum"], fx[f"log_{which}_abs"]
        assert want.shape == (BH, outer) and want.dtype == np.float64
        bound = fp16_bound(want, sumabs)
        assert (np.abs(C64[:, 0] - want) <= 1e-9 * (1 + sumabs)).all(), which
        assert (np.abs(C16[:, 0].astype(np.float64) - want) <= bound).all(), which
        assert not C16[:, 1:].any()


@pytest.mark.parametrize("name", RAN)
def test_every_logged_operator_call(fixtures, name):
    """The whole call log: every step with a compressed part issues one key and one value call, in that order, with the 8 padded rows
    (:273, :313), the flat cache arrays of that step's compressed length, and the scalars of :274 / :314; a step without one issues none."""
    fx = fixtures[name]
    s = fx.spec
    D, BH, heads, groups = s["D"], s["bsz"] * s["Hq"], s["bsz"] * s["Hkv"], s["Hq"] // s["Hkv"]
    calls = fx.meta["all_calls"]
    want_steps = [i for i in range(fx.recorded_steps) if fx["compressed_length"][i] != 0]
    assert [(c["step"], c["name"]) for c in calls] == [(i, n) for i in want_steps for n in ("key", "value")]
    for c in calls:
        T = int(fx["compressed_length"][c["step"]])           # the compressed length BEFORE the step's own trigger
        tiles = T * D // 64
        numel = lambda shape: int(np.prod(shape))
        assert numel(c["shapes"][0]) == heads * tiles and numel(c["shapes"][2]) == heads * (tiles + 1) and c["shapes"][3] == [heads]
        assert len(c["shapes"][1]) == 1 and c["shapes"][1][0] % 8 == 0    # one flat stream; every head's share a whole number of uint4
        assert c["dtypes"] == ["torch.int64", "torch.float16", "torch.int32", "torch.int32", "torch.float16"]
        if c["name"] == "key":
            assert c["shapes"][4] == [BH, 8, D] and c["scalars"] == [T, D, BH, groups]
        else:
            assert c["shapes"][4] == [BH, 8, T] and c["scalars"] == [D, T, BH, groups]
    assert fx.meta["operator_log"] == [dict({k: c[k] for k in ("name", "shapes", "dtypes", "scalars")}, rows_1_to_7_zero=True) for c in calls[-2:]]


# ---- the checks themselves refuse bad input (synthetic numbers, no product code) ----------------------------------------------------
def test_within_refuses_an_output_just_past_the_bound():
    model = torch.tensor([[1.0, -2.0, 0.5, 0.0]], dtype=torch.float64)
    b_out = torch.tensor([[1e-3, 2e-3, 1e-3, 1e-4]], dtype=torch.float64)
    b_rec = torch.tensor([[5e-4, 5e-4, 5e-4, 5e-5]], dtype=torch.float64)
    rec = model + 0.9 * b_rec
    ok, rm, rr = fg.within(model + 0.999 * b_out, rec, b_out, b_rec, model)
    assert ok and 0.99 < rm <= 1.0 and rr <= 1.0
    bad = model.clone()
    bad[0, 2] += 1.001 * b_out[0, 2]                      # one element just past its own bound; every other element exact
    ok, rm, rr = fg.within(bad, rec, b_out, b_rec, model)
    assert not ok and 1.0 < rm < 1.01
    # inside the model's bound but too far from the recording: the recording on one side, the output on the other
    rec2 = model - b_rec
    out2 = model.clone()
    out2[0, 1] += 0.9 * b_out[0, 1]
    assert fg.within(out2, rec2, b_out, b_rec, model)[0]
    rec3 = model.clone()
    rec3[0, 1] -= 2.0 * b_rec[0, 1] + 0.2 * b_out[0, 1]   # (a recording this far out would itself fail test_recorded_outputs)
    ok, rm, rr = fg.within(out2, rec3, b_out, b_rec, model)
    assert not ok and rm <= 1.0 < rr
    nan = model.clone()
    nan[0, 0] = float("nan")
    assert not fg.within(nan, rec, b_out, b_rec, model)[0]


def test_loader_refuses_a_compressed_length_off_by_256():
    spec = dict(L0=538, steps=8)
    cl, wl, kv = fg.closed_form(538, 8)
    good = dict(out=np.zeros((8, 1, 4), np.uint16), compressed_length=cl, window_len=wl, kv_seq_len=kv)
    fg.validate(good, spec)
    for step, delta in ((0, 256), (6, -256), (8, 256)):
        bad = dict(good, compressed_length=cl.copy())
        bad["compressed_length"][step] += delta
        with pytest.raises(ValueError, match="compressed_length"):
            fg.validate(bad, spec)
    early = dict(good, compressed_length=cl.copy(), window_len=wl.copy())   # the trigger one step early, window consistent with it
    early["compressed_length"][5] += 256
    early["window_len"][5] -= 256
    with pytest.raises(ValueError):
        fg.validate(early, spec)
    with pytest.raises(ValueError, match="window_len"):
        fg.validate(dict(good, window_len=wl + 1), spec)

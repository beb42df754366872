"""GPU: the decode hook, in every configuration, held to runs recorded from the reference's own forward (tests/golden/forward_*.npz;
tests/forward_golden_util.py says what a fixture holds, tests/test_forward_golden.py checks the recordings themselves on the CPU).

Every run builds the cache from the recorded prefill rows, then decodes step by step with the recorded q / k / v and mask.  After every
step compressed_length, kv_seq_len and the window length equal the recording, and the output lies within the float64 model's bound of
the model and within the sum of both bounds of the recorded output (fused: hook_model's bound; the unfused sequences: reference_bound).
After the prefill and after the trigger step the cache, converted by its own to_reference(), and the windows' live rows equal the
recorded arrays bit for bit.

Worst ratios of one MI355X run, |out - model| / bound and |out - recorded| / (bound + reference_bound), over all steps:
see DESIGN.md §2 (each test prints its own)."""
import numpy as np
import pytest
import torch

from tests import forward_golden_util as fg
from tests.util import fp16_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

D128 = {
    "reference": dict(api="reference"),
    "native": dict(api="native"),
    "fused": dict(api="fused"),
    "fused-arena": dict(api="fused", arena=True),
    "fused-two_launch": dict(api="fused", structure="two_launch"),
}
ENGINES = {f"fused-{e}": dict(api="fused", engine=e) for e in ("dot2", "valu", "mfma")}
D64 = {
    "fused": dict(api="fused"),
    "fused-extents": dict(api="fused", hd64_extents=True),
    "fused-raw_prefill": dict(api="fused", hd64_raw_prefill=True),
}
RUNS = [(n, c) for n in ("append", "first", "mask") for c in D128] + [("mask", c) for c in ENGINES] + [("d64", c) for c in D64]


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return {name: fg.load(golden_dir, name) for name in fg.SCENARIOS}


def _attention(spec, kwargs):
    from mustafar_amd.hook import MustafarAttention, MustafarConfig
    return MustafarAttention(MustafarConfig(num_attention_heads=spec["Hq"], num_key_value_heads=spec["Hkv"], head_dim=spec["D"],
                                            k_sparsity=fg.K_SPARSITY, v_sparsity=fg.V_SPARSITY, residual_length=fg.RESIDUAL, **kwargs))


def _reference_arrays(cache):
    """A cache of any kind -> (bmp [heads, tiles], idx [heads, tiles + 1], the concatenated stream as bits, nz_offset), numpy, through
    the cache's own to_reference(); one that grew by an extent is consolidated first (and must give the same without)."""
    from mustafar_amd.hook import _flat_stream
    variants = [cache]
    if hasattr(cache, "to_reference"):
        variants = [cache.to_reference()]
        if cache.extents:
            variants.append(cache.consolidate().to_reference())
    got = []
    for bmp, idx, nz, off in variants:
        heads = len(nz)
        assert bmp.dtype == torch.int64 and idx.dtype == torch.int32 and off.dtype == torch.int32
        got.append((bmp.reshape(heads, -1).cpu().numpy(), idx.reshape(heads, -1).cpu().numpy(),
                    _flat_stream([bmp, idx, nz, off]).cpu().numpy().view(np.uint16), off.cpu().numpy()))
    for other in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got[-1], other)), "to_reference() and consolidate().to_reference() differ"
    return got[-1]


def _window(w):
    return (w.view() if hasattr(w, "view") and not isinstance(w, torch.Tensor) else w).cpu().numpy().view(np.uint16)


def _check_state(fx, past, after, tag):
    """The cache and windows of `past` against the snapshot recorded after step `after` (-1: the prefill), bit for bit."""
    snap = fx.snapshot(after)
    for side, cache, win in (("k", past[0], past[1]), ("v", past[2], past[3])):
        assert np.array_equal(_window(win), snap[f"{side}_win"]), f"{tag}: {side} window rows differ from the recording after step {after}"
        if f"{side}_bmp" not in snap:
            assert cache is None
            continue
        for name, got in zip(("bmp", "idx", "nz", "nz_offset"), _reference_arrays(cache)):
            want = snap[f"{side}_{name}"]
            assert got.shape == want.shape and np.array_equal(got, want), f"{tag}: {side} {name} differs from the recording after step {after}"


def _window_len(past):
    return past[1].len if hasattr(past[1], "len") else past[1].shape[2]


@pytest.mark.parametrize("name,config", RUNS)
def test_hook_follows_the_recorded_forward(fixtures, name, config):
    fx = fixtures[name]
    s = fx.spec
    kwargs = (D64 if s["D"] == 64 else {**D128, **ENGINES})[config]
    fused = kwargs["api"] == "fused"
    attn = _attention(s, kwargs)
    _, K, V, _ = fx.inputs()
    tag = f"{name} / {config}"
    past = attn.build_cache(K[:, :, :s["L0"]].to(DEV), V[:, :, :s["L0"]].to(DEV))
    assert (past[4], past[5], _window_len(past)) == (fx["compressed_length"][0], fx["kv_seq_len"][0], fx["window_len"][0])
    _check_state(fx, past, -1, tag)
    snaps = set(fx["snap_after"].tolist())
    worst_model = worst_rec = 0.0
    assert fx.recorded_steps == s["steps"]
    for i in range(fx.recorded_steps):
        m = fg.step_model(fx, i)
        mask = m["mask"].contiguous().to(DEV) if m["mask"] is not None else None
        out, past = attn.decode(m["q"].to(DEV), m["k"].to(DEV), m["v"].to(DEV), past, attention_mask=mask)
        assert out.shape == (s["bsz"], s["Hq"], 1, s["D"]) and out.dtype == torch.float16
        assert (past[4], past[5], _window_len(past)) == (fx["compressed_length"][i + 1], fx["kv_seq_len"][i + 1], fx["window_len"][i + 1]), \
            f"{tag}: bookkeeping after step {i}"
        bound = m["hook_bound"] if fused else m["ref_bound"]
        ok, rm, rr = fg.within(out, m["rec"], bound, m["ref_bound"], m["model"])
        print(f"{tag} step {i} (C {m['C']}, kv {m['kv']}): |out - model| / bound {rm:.3f}, |out - recorded| / (bound + reference_bound) {rr:.3f}")
        worst_model, worst_rec = max(worst_model, rm), max(worst_rec, rr)
        assert ok, f"{tag} step {i}: |out - model| / bound = {rm:.3f}, |out - recorded| / (bound + reference_bound) = {rr:.3f}"
        if i in snaps:
            _check_state(fx, past, i, tag)
    print(f"RATIOS {tag}: model {worst_model:.3f} recorded {worst_rec:.3f}")


@pytest.mark.parametrize("config", ["reference", "native", "fused", "fused-arena"])
def test_short_prefill_keeps_its_window(fixtures, config):
    """The one place where the hook leaves the reference on purpose.  The recording says what the reference does with a
    30-token prefill: :416 leaves compressed_length = -256 and the first decode step hands that to the key operator.  The hook clamps at 0
    (build_cache) and, when :324 comes true at kv = 32 with a 32-row window, keeps the window (the guard in decode / trigger_due): it
    must not raise, compress nothing, and give dense attention over the raw rows."""
    fx = fixtures["short"]
    s = fx.spec
    assert fx.recorded_steps == 0 and fx["compressed_length"].tolist() == [-256]
    assert fx.meta["result"] == "OperatorRefused at step 0: mustafar_key_formulation called with compressed_length -256"
    kwargs = D128[config]
    attn = _attention(s, kwargs)
    _, K, V, _ = fx.inputs()
    past = attn.build_cache(K[:, :, :30].to(DEV), V[:, :, :30].to(DEV))
    assert past[0] is None and past[2] is None and (past[4], past[5], _window_len(past)) == (0, 30, 30)
    assert np.array_equal(_window(past[1]), fx.snapshot(-1)["k_win"]) and np.array_equal(_window(past[3]), fx.snapshot(-1)["v_win"])
    for i in range(s["steps"]):
        m = fg.step_model(fx, i, C=0)
        out, past = attn.decode(m["q"].to(DEV), m["k"].to(DEV), m["v"].to(DEV), past)
        kv = 31 + i
        assert past[0] is None and past[2] is None and (past[4], past[5], _window_len(past)) == (0, kv, kv)   # kv = 32: :324 holds, nothing compressed
        assert np.array_equal(_window(past[1]), K[:, :, :kv].numpy().view(np.uint16))
        bound = m["hook_bound"] if kwargs["api"] == "fused" else m["ref_bound"]
        ratio = float(((out.cpu().double() - m["model"]).abs() / bound).max())
        print(f"short / {config} step {i} (kv {kv}): |out - model| / bound {ratio:.3f}")
        assert torch.isfinite(out).all() and ratio <= 1.0
    assert (31 + s["steps"] - 1 - fg.RESIDUAL - 0) % 256 == 0   # the last step is the one at which :324 came true


@pytest.mark.parametrize("name", ["append", "first", "mask"])
@pytest.mark.parametrize("module", ["ctypes", "compiled"])
def test_logged_operator_calls_replayed(fixtures, name, module):
    """The last step's two operator calls as the reference's forward issued them (the 8 padded rows, the logged shapes, dtypes and scalars, the
    flat cache of the last snapshot) through `mustafar_amd.mustafar_package` and the compiled drop-in of the reference's name."""
    fx = fixtures[name]
    s = fx.spec
    if module == "compiled":
        from mustafar_amd import hook
        ops = hook._operator_module()
        assert ops.__file__.endswith(".so"), "the compiled extension must be the one under test"
    else:
        from mustafar_amd import mustafar_package as ops
    snap = fx.snapshot(fx.recorded_steps - 1)
    T, D, BH, groups = int(fx["compressed_length"][-1]), s["D"], s["bsz"] * s["Hq"], s["Hq"] // s["Hkv"]
    ws = torch.zeros(1, dtype=torch.float16, device=DEV)
    for c in fx.meta["operator_log"]:
        which, side = c["name"], c["name"][0]
        inner, outer = (D, T) if which == "key" else (T, D)
        B = torch.zeros((BH, 8, inner), dtype=torch.float16)
        B[:, 0] = torch.from_numpy(fx[f"log_{which}_b"].view(np.float16).copy())
        t = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a)).reshape(shape).to(DEV)
        bmp, nz, idx, off = (t(snap[f"{side}_bmp"], c["shapes"][0]), t(snap[f"{side}_nz"].view(np.float16), c["shapes"][1]),
                             t(snap[f"{side}_idx"], c["shapes"][2]), t(snap[f"{side}_nz_offset"], c["shapes"][3]))
        B = B.to(DEV)
        assert list(B.shape) == c["shapes"][4] and [str(x.dtype) for x in (bmp, nz, idx, off, B)] == c["dtypes"] and c["rows_1_to_7_zero"]
        if which == "key":
            assert c["scalars"] == [T, D, BH, groups]
            out = ops.mustafar_key_formulation(bmp, nz, idx, off, B, *c["scalars"])
        else:
            assert c["scalars"] == [D, T, BH, groups]
            out = ops.mustafar_value_formulation(bmp, nz, idx, off, B, ws, *c["scalars"])
        assert out.shape == (BH, 8, outer) and out.dtype == torch.float16
        got = out.cpu().numpy()
        want, sumabs = fx[f"log_{which}_sum"], fx[f"log_{which}_abs"]
        ratio = float((np.abs(got[:, 0].astype(np.float64) - want) / fp16_bound(want, sumabs)).max())
        print(f"{name} / {module} {which}: row 0 |out - logged sum| / fp16_bound {ratio:.3f}")
        assert np.isfinite(got).all() and ratio <= 1.0
        assert not got[:, 1:].any(), "rows 1-7 of the padded operand are zero: so must their results be"

"""No GPU: the plans of the long decode sessions (tests/session_plan.py) meet the conditions the GPU test relies on, the executor and its
truth bookkeeping (tests/session_util.py) pass every plan on the dense stand-in of tests/session_fake.py with every ratio <= 1, and every
defect of the stand-in is caught by the check named here -- the mutant evidence for the harness."""
import pytest
import torch

from tests import session_fake as sf
from tests import session_plan as sp
from tests import session_util as sx

DECODE = ("step", "multi", "split", "multi_split")


def _fake(kind, defect=None):
    k = sp.KINDS[kind]
    return sf.FakeAttention(sp.HKV * k["groups"], sp.HKV, k["head_dim"], k["k_sparsity"], k["v_sparsity"], defect=defect)


def _session(kind, seed, defect=None):
    return sx.Session(kind, seed, _fake(kind, defect), torch.device("cpu"), sf.make_shared, sf.make_segment)


def test_the_seed_list_covers_every_kind_twice_and_every_start():
    assert len(sp.SESSIONS) == 16 and {k for k, _ in sp.SESSIONS} == set(sp.KINDS)
    for D in (64, 128):
        heads = {(h["start"], bool(h["pad"])) for k, s in sp.SESSIONS if sp.KINDS[k]["head_dim"] == D for h in [sp.header(k, s)]}
        assert heads == {(250, False), (250, True), (300, False), (300, True)}


@pytest.mark.parametrize("kind,seed", sp.SESSIONS)
def test_a_plan_is_deterministic_and_meets_its_conditions(kind, seed):
    k, ops = sp.KINDS[kind], sp.plan(kind, seed)
    assert ops == sp.plan(kind, seed)
    per = 64 // k["groups"]
    # the length rules, restated: no call steps over a trigger point, every trigger fires exactly where it is due
    h = sp.header(kind, seed)
    L = h["start"]
    C = max(0, (L - sp.R) // 256 * 256)
    holes = [set(), set(range(h["pad"]))]
    fired, hole_trigger, after_hole_trigger, deep_split = [], None, 0, 0
    for i, op in enumerate(ops):
        name = op["op"]
        if name in DECODE:
            n = op.get("n_q", 1)
            assert all((L + j + 1 - sp.R - C) % 256 or L + j + 1 - C < 256 for j in range(n - 1)), f"op {i} steps over a trigger point"
            L += n
            assert name not in ("multi", "multi_split") or 1 <= n <= max(20, per + 4)
            if name == "split" and "s" in op["frozen"]:
                assert not any(holes), f"op {i}: decode_split with a shared entry while a hole exists"
            if hole_trigger is not None:
                after_hole_trigger += 1
            if name == "multi_split" and len(fired) >= 2 and any(r < C for hs in holes for r in hs):
                deep_split += 1
        elif name == "accept":
            n_keep = op["n_q"] - op["rejected"] if op["keep"] is None else len(op["keep"][0])
            first = L - op["n_q"]
            L = first + n_keep
            for b, rows in enumerate(op["new_holes"]):
                assert all(first <= r < L for r in rows)
                holes[b] |= set(rows)
        due = (L - sp.R - C) % 256 == 0 and L - C >= 256
        if name == "run_triggers":
            assert due and op["fired"] and ops[i - 1].get("defer")
        elif name in ("multi", "multi_split"):      # appends and never compresses: its accept closes it
            assert not op["fired"] and op["last_row_is_point"] == due
        elif due:
            assert op["fired"] != bool(op.get("defer")), f"op {i}: a trigger is due"
        else:
            assert not op["fired"]
        if op["fired"]:
            moved = sum(1 for hs in holes for r in hs if C <= r < C + 256)
            assert moved == op["holes_compressed"]
            if moved and hole_trigger is None:
                hole_trigger = i
            C += 256
            fired.append(i)
        assert (op["L"], op["C"], op["W"]) == (L, C, L - C), f"op {i}"
    assert len(fired) >= 4
    # a trigger fired by accept() after a multi whose last row is the trigger point
    assert any(op["op"] == "accept" and op["fired"] and op["closes"] == "multi" and ops[i - 1]["last_row_is_point"]
               for i, op in enumerate(ops))
    # an accept that ends exactly one row short of a trigger point, then a step that fires
    assert any(op["op"] == "accept" and op["L"] == op["C"] + sp.R + 255 and ops[i + 1]["op"] == "step" and ops[i + 1]["fired"]
               for i, op in enumerate(ops[:-1]))
    assert sum(1 for op in ops if op["op"] == "multi" and op["n_q"] > per and op["mask"] in ("causal", "tree")) >= 2
    assert any(op["op"] == "accept" and op["unequal"] and any(op["new_holes"]) for op in ops)
    assert hole_trigger is not None and after_hole_trigger >= 3
    if k["split"]:
        assert sum(1 for op in ops if op["op"] == "split") >= 5 and sum(1 for op in ops if op["op"] == "multi_split") >= 5
        assert deep_split >= 1
    else:
        assert not any(op["op"] in ("split", "multi_split") for op in ops)
    if k["layers"] == 2:
        runs = [op for op in ops if op["op"] == "run_triggers"]
        assert len(runs) >= 2 and any(op["pool"] for op in runs)
        assert any(ops[i - 1]["op"] == "accept" for i, op in enumerate(ops) if op["op"] == "run_triggers")
    if k["small_table"]:
        assert any(op["fired"] and op["full_table"] for op in ops)


@pytest.mark.parametrize("kind,seed", sp.SESSIONS)
def test_the_clean_stand_in_passes_the_plan(kind, seed):
    rep = _session(kind, seed).run()
    print(f"{kind} seed {seed}: {rep['ops']} ops, worst ratios {rep['worst']}, negative control {rep['control']:.1f}")
    assert rep["worst"] and all(r <= 1.0 for r in rep["worst"].values()) and rep["control"] > 1.0


# defect -> (the session that shows it, the check that must catch it)
CAUGHT = {
    "rejected_visible": ("ext64", 6, "ratio"),
    "keep_skips_v": ("ext64", 6, "ratio"),
    "trigger_late": ("ext64", 6, "lengths"),
    "trigger_255": ("ext64", 6, "twin_cache"),
    "split_mask_left": ("ext64", 6, "ratio"),
    "hole_unmasked_compressed": ("ext64", 6, "ratio"),
    "chunk_mask_rows": ("ext64", 1, "ratio"),
    "skip_layer": ("ext64", 1, "lengths"),
}


def test_every_defect_has_a_case():
    assert set(CAUGHT) == set(sf.DEFECTS)


@pytest.mark.parametrize("defect", sf.DEFECTS)
def test_a_defect_of_the_stand_in_is_caught(defect):
    kind, seed, check = CAUGHT[defect]
    with pytest.raises(sx.SessionFailure) as e:
        _session(kind, seed, defect).run()
    print(f"{defect}: {e.value}")
    assert e.value.check == check

"""Helpers of tests/test_gpu_multi_query_mask.py: masks for the several-token decode call (ABI 114), the call of the masked C entry point
over the operands of tests/test_gpu_multi_query.py's `Call`, and the models with a mask row per query token.

Every mask a test hands to the library is a view into a LARGER tensor whose other elements are NaN -- planes behind the planes of the
batch, rows behind the rows of the call, columns before and behind the columns of the row, the view starting at an odd element: a plane,
row or column taken from the wrong place, or a read past the end of a row, poisons the output."""
import ctypes
import math

import torch

from tests import exact_data as xd
from tests import partial_util as pu
from tests.hd64_util import DEV

NEG = torch.finfo(torch.float16).min
NAN = float("nan")


def housed(mask, lead=3, tail=5):
    """`mask` [planes, rows, columns] (any device) as a view of a NaN tensor [planes + 2, rows + 1, lead + columns + tail] on the GPU,
    starting at the odd element `lead`: the same values, rows and planes the wider tensor's strides apart."""
    P, R, Cn = mask.shape
    wide = torch.full((P + 2, R + 1, lead + Cn + tail), NAN, dtype=torch.float16, device=DEV)
    view = wide[:P, :R, lead:lead + Cn]
    view.copy_(mask)
    assert view.data_ptr() % 4 == 2 * (lead % 2) and view.stride(2) == 1
    return view


def call_masked(c, q, mask, heads_per_mask):
    """mustafar_decode_multi_query_masked over the operands of `c` (tests/test_gpu_multi_query.py: Call); mask: a device view
    [planes, 1 or n_q, T + window_len] with unit stride along a row.  Returns (out, lse) -- c's own tensors, overwritten."""
    p = lambda t: t.data_ptr() if t is not None else None
    kv, vv = (ctypes.byref(c.kv), ctypes.byref(c.vv)) if c.C else (None, None)
    assert mask.shape[2] == c.C + c.w_len and mask.shape[0] * heads_per_mask == c.B * c.Hkv and mask.stride(2) == 1
    c.out.fill_(NAN)
    c.lse.fill_(NAN)
    err = c.L.mustafar_decode_multi_query_masked(torch.cuda.current_stream().cuda_stream, kv, vv, c.C, None, None, c.C, c.B * c.Hkv, c.groups,
                                                 c.n_q, q.data_ptr(), c.kw.data_ptr(), c.vw.data_ptr(), p(c.kn), p(c.vn), c.w_len, c.cap,
                                                 c.out.data_ptr(), c.lse.data_ptr(), c.ws.data_ptr(), ctypes.c_float(math.sqrt(c.Dd)), c.Dd,
                                                 mask.data_ptr(), mask.stride(0), mask.stride(1), mask.shape[1], heads_per_mask)
    assert err == 0
    return c.out, c.lse


def per_head(mask, B, Hq, heads_per_plane):
    """[planes, rows, columns] -> [B, Hq, rows, columns]: plane p serves `heads_per_plane` consecutive q heads of the [B * Hq] heads."""
    P, R, Cn = mask.shape
    assert P * heads_per_plane == B * Hq
    return mask[:, None].expand(P, heads_per_plane, R, Cn).reshape(B, Hq, R, Cn)


def model_ratios(out, lse, q, Kp, Vp, first, groups, mask4):
    """max |out - hook_model| / bound and |lse - lse_model| / bound over the tokens of a call: token j sees rows [0, first + j + 1) of Kp /
    Vp under row j of mask4 [B, 1 or Hq, 1 or n_q, >= first + n_q] (its only row when it has one), None: no mask."""
    r_out = r_lse = 0.0
    for j in range(q.shape[2]):
        Lj = first + j + 1
        mj = None
        if mask4 is not None:
            row = j if mask4.shape[2] > 1 else 0
            mj = mask4[:, :, row:row + 1, :Lj]
        want, bound = xd.hook_model(q[:, :, j:j + 1], Kp[:, :, :Lj], Vp[:, :, :Lj], groups, mask=mj)
        r = (out[:, :, j:j + 1].double() - want).abs() / bound
        r_out = max(r_out, float(r.max()) if torch.isfinite(r).all() else float("inf"))
        want_l, bound_l = pu.lse_model(q[:, :, j:j + 1], Kp[:, :, :Lj], groups, mask=mj)
        r_lse = max(r_lse, pu.lse_ratio(lse[:, :, j], want_l, bound_l))
    return r_out, r_lse


def assert_models(out, lse, q, Kp, Vp, first, groups, mask4, what):
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), f"{what}: NaN / Inf in the outputs"
    r_out, r_lse = model_ratios(out, lse, q, Kp, Vp, first, groups, mask4)
    print(f"{what}: |out - model| / bound = {r_out:.3f}, |lse - model| / bound = {r_lse:.3f}")
    assert r_out <= 1.0 and r_lse <= 1.0, f"{what}: out {r_out:.3f}, lse {r_lse:.3f}"


# ---- masks [planes, rows, columns] (CPU, fp16) -------------------------------------------------------------------------------------------
def zeros(P, rows, columns):
    return torch.zeros((P, rows, columns), dtype=torch.float16)


def left_padding(pads, columns):
    """One row per plane: the first pads[p] columns at finfo.min."""
    m = zeros(len(pads), 1, columns)
    for p, n in enumerate(pads):
        m[p, 0, :n] = NEG
    return m


def ancestors(parent):
    """[n, n] bool: [j, i] iff node i is node j or one of its ancestors (parent[j] < j, -1: a root)."""
    n = len(parent)
    a = torch.zeros((n, n), dtype=torch.bool)
    for j in range(n):
        i = j
        while i >= 0:
            a[j, i] = True
            i = parent[i]
    return a


def tree_mask(P, parent, first, holes=None):
    """[P, n, first + n]: row j is 0 on the old columns and on node j's ancestors and itself among the n new ones, finfo.min on the other
    new ones; holes[p]: old columns at finfo.min in every row of plane p."""
    n = len(parent)
    m = zeros(P, n, first + n)
    m[:, :, first:] = torch.where(ancestors(parent), 0.0, NEG).half()
    for p, hs in enumerate(holes or []):
        m[p][:, list(hs)] = NEG
    return m


def random_tree(n, gen):
    """parent[j] < j, node 0 the root."""
    return [-1] + [int(torch.randint(0, j, (1,), generator=gen)) for j in range(1, n)]

"""CPU: the error contract of the host layer. Every invalid call below raises the exception type and the
full message written next to it in EXPECT, op wrappers (ops.py) and regional model methods (models.py)
alike. Most of the ops' checks sit behind the device gate (ops._dev / ops._dev_typed), which only a GPU
passes; here the gate alone is taken out, so that a CPU (or meta) tensor goes through while the tensor-type,
dtype and contiguity behaviour stays, and the library is replaced by an object that fails the test when
touched: a check that got lost shows as a failure in Python, nothing is ever launched. No GPU needed."""
import pytest
import torch

from arbitrarystyletransfer_amd import models, ops
from arbitrarystyletransfer_amd._lib import HipOpError

f32, i32, i64, u8, i8 = torch.float32, torch.int32, torch.int64, torch.uint8, torch.int8


def Z(*shape, dtype=f32):
    return torch.zeros(shape, dtype=dtype)


def M(*shape, dtype=f32):
    """A tensor too large to allocate, on the meta device (the stubbed gate lets it through)."""
    return torch.empty(shape, dtype=dtype, device="meta")


class _NoLibrary:
    """In place of ops.lib: any use of the library is a lost check."""

    def __call__(self):
        return self

    def __getattr__(self, name):
        pytest.fail(f"the call reached the library ({name}): a host-side check is missing")


def _dev_without_gate(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.dtype != torch.float32:
        raise HipOpError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _dev_typed_without_gate(t, name, dtype, *args, **kwargs):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.dtype != dtype:
        raise HipOpError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(ops, "_dev", _dev_without_gate)
    monkeypatch.setattr(ops, "_dev_typed", _dev_typed_without_gate)
    monkeypatch.setattr(ops, "lib", _NoLibrary())
    monkeypatch.setattr(ops, "stream_ptr", lambda device: 0)   # no check: a CPU device has no stream


# ---- the ops ---------------------------------------------------------------------------------------------

ROWS = []   # (id, call)


def row(rid, call):
    ROWS.append((rid, call))


A = Z(2, 4, 5, 6)   # the valid first map of every pair below

# the pair check: two NCHW maps, equal C, second batch N or 1, not empty (style swap: sides of at least 3)
PAIR_OPS = {
    "efdm": lambda a, b: ops.efdm(a, b),
    "wct": lambda a, b: ops.wct(a, b),
    "patch_match": lambda a, b: ops.patch_match(a, b),
    "patch_gather": lambda a, b: ops.patch_gather(b, Z(2, 3, 4, dtype=i32), a),
    "style_swap": lambda a, b: ops.style_swap(a, b),
    "cosine_match": lambda a, b: ops.cosine_match(a, b),
    "remd_loss": lambda a, b: ops.remd_loss(a, b),
    "selfsim_loss": lambda a, b: ops.selfsim_loss(a, b),
    "cx_loss": lambda a, b: ops.cx_loss(a, b),
}
for _name, _op in PAIR_OPS.items():
    row(f"{_name}-rank", lambda op=_op: op(A, Z(4, 5, 6)))
    row(f"{_name}-channels", lambda op=_op: op(A, Z(2, 3, 5, 6)))
    row(f"{_name}-batch", lambda op=_op: op(Z(3, 4, 5, 6), A))
    row(f"{_name}-empty", lambda op=_op: op(A, Z(2, 4, 0, 6)))
    if _name in ("patch_match", "patch_gather", "style_swap"):
        row(f"{_name}-side", lambda op=_op: op(A, Z(2, 4, 2, 6)))
        row(f"{_name}-side-first", lambda op=_op: op(Z(2, 4, 5, 2), A))
row("efdm-rank-first", lambda: ops.efdm(Z(4, 5, 6), A))
row("efdm-empty-first", lambda: ops.efdm(Z(2, 4, 5, 0), A))
row("efdm-not-a-tensor", lambda: ops.efdm(A, [[1.0]]))
row("efdm-first-not-a-tensor", lambda: ops.efdm(None, [[1.0]]))

# the limits that the losses add to the pair check
for _name in ("cosine_match", "remd_loss", "selfsim_loss", "cx_loss"):
    _op = PAIR_OPS[_name]
    row(f"{_name}-remd-channels", lambda op=_op: op(M(1, 1025, 2, 2), M(1, 1025, 2, 2)))
    row(f"{_name}-remd-pixels", lambda op=_op: op(M(1, 2, 2049, 2048), M(1, 2, 2049, 2048)))
    row(f"{_name}-remd-pixels-second", lambda op=_op: op(M(1, 2, 2, 2), M(1, 2, 2049, 2048)))
    row(f"{_name}-remd-batch", lambda op=_op: op(M(65536, 2, 2, 2), M(1, 2, 2, 2)))
row("remd_loss-branch", lambda: ops.remd_loss(A, A, _branch=3))
row("selfsim_loss-shapes", lambda: ops.selfsim_loss(A, Z(2, 4, 6, 5)))
row("selfsim_loss-shapes-batch", lambda: ops.selfsim_loss(A, Z(1, 4, 5, 6)))
row("selfsim_loss-pixels", lambda: ops.selfsim_loss(M(1, 2, 129, 128), M(1, 2, 129, 128)))
row("selfsim_colsum-pixels", lambda: ops.selfsim_colsum(M(1, 2, 129, 128), M(1, 129, 128)))
row("selfsim_colsum-inv_norm", lambda: ops.selfsim_colsum(A, Z(2, 5, 5)))
row("selfsim_pairs-r_x", lambda: ops.selfsim_pairs(A, A, Z(2, 5, 6), Z(2, 5, 6), Z(2, 5, 6, dtype=i32), Z(2, 5, 6)))
row("cx_loss-pixels", lambda: ops.cx_loss(M(1, 2, 129, 128), M(1, 2, 2, 2)))
row("cx_loss-pixels-second", lambda: ops.cx_loss(M(1, 2, 2, 2), M(1, 2, 129, 128)))
row("cx_loss-h-zero", lambda: ops.cx_loss(A, A, h=0.0))
row("cx_loss-h-negative", lambda: ops.cx_loss(A, A, h=-0.5))
row("cx_loss-h-inf", lambda: ops.cx_loss(A, A, h=float("inf")))
row("cx_loss-h-nan", lambda: ops.cx_loss(A, A, h=float("nan")))
row("cx_center-pixels", lambda: ops.cx_center(M(1, 2, 129, 128), M(1, 2, 2, 2)))
row("cx_rowsum-h", lambda: ops.cx_rowsum(A, A, Z(2, 5, 6), Z(2, 5, 6), Z(2, 5, 6), h=0.0))
row("cx_rowsum-inv_y", lambda: ops.cx_rowsum(A, A, Z(2, 5, 6), Z(2, 5, 5), Z(2, 5, 6)))
row("cx_colmax-row_sum", lambda: ops.cx_colmax(A, A, Z(2, 5, 6), Z(2, 5, 6), Z(2, 5, 6), Z(2, 5, 6, dtype=i32)))

# moment_loss: its map, its limits, and the target statistics
X = Z(2, 3, 2, 2)
row("moment_loss-rank", lambda: ops.moment_loss(Z(3, 2, 2), Z(1, 3), Z(1, 3, 3)))
row("moment_loss-empty", lambda: ops.moment_loss(Z(2, 3, 0, 2), Z(1, 3), Z(1, 3, 3)))
row("moment_loss-channels", lambda: ops.moment_loss(M(1, 1025, 2, 2), M(1, 1025), M(1, 1025, 1025)))
row("moment_loss-one-pixel", lambda: ops.moment_loss(Z(2, 3, 1, 1), Z(1, 3), Z(1, 3, 3)))
row("moment_loss-samples", lambda: ops.moment_loss(M(32768, 2, 2, 2), M(1, 2), M(1, 2, 2)))
row("moment_loss-y_mean-batch", lambda: ops.moment_loss(X, Z(3, 3), Z(3, 3, 3)))
row("moment_loss-y_mean-rank", lambda: ops.moment_loss(X, Z(3), Z(1, 3, 3)))
row("moment_loss-y_mean-not-a-tensor", lambda: ops.moment_loss(X, None, Z(1, 3, 3)))
row("moment_loss-y_mean-channels", lambda: ops.moment_loss(X, Z(1, 4), Z(1, 3, 3)))
row("moment_loss-y_mean-dtype", lambda: ops.moment_loss(X, Z(2, 3, dtype=torch.float64), Z(2, 3, 3)))
row("moment_loss-y_cov-shape", lambda: ops.moment_loss(X, Z(2, 3), Z(1, 3, 3)))
row("moment_loss-y_cov-dtype", lambda: ops.moment_loss(X, Z(2, 3), Z(2, 3, 3, dtype=torch.float64)))
row("moment_loss-y_cov-not-a-tensor", lambda: ops.moment_loss(X, Z(2, 3), None))
row("moment_stats-one-pixel", lambda: ops.moment_stats(Z(2, 3, 1, 1)))


# the state of the four backward functions: every element with a wrong dtype and a wrong shape or count
def _state_rows(name, good, checked, call, other=f32, exact=True):
    """good: {element name: (shape, dtype)} in the order of the state; checked: the names the op reads."""
    def state(**bad):
        return tuple(bad[k] if k in bad else Z(*shape, dtype=dt) for k, (shape, dt) in good.items())
    for k in checked:
        shape, dt = good[k]
        row(f"{name}-{k}-dtype", lambda k=k, shape=shape, dt=dt: call(state(
            **{k: Z(*shape, dtype=other if dt != other else i32)})))
        row(f"{name}-{k}-shape", lambda k=k, shape=shape, dt=dt: call(state(**{k: Z(*shape, 2, dtype=dt)})))
    if exact:
        row(f"{name}-state-short", lambda: call(state()[:-1]))
        row(f"{name}-state-long", lambda: call(state() + (Z(1),)))
    row(f"{name}-state-element-not-a-tensor", lambda: call(state(**{checked[0]: None})))
    row(f"{name}-state-not-a-tuple", lambda: call(None))
    return state


RX, RY = Z(2, 3, 2, 2), Z(1, 3, 2, 3)     # n = 2, m = 4; ns = 1, p = 6
REMD_STATE = {"inv_x": ((2, 2, 2), f32), "inv_y": ((1, 2, 3), f32), "row_min": ((2, 2, 2), f32),
              "row_index": ((2, 2, 2), i32), "col_min": ((2, 2, 3), f32), "col_index": ((2, 2, 3), i32)}
_remd_state = _state_rows("remd_loss_backward", REMD_STATE, list(REMD_STATE),
                          lambda st: ops.remd_loss_backward(RX, RY, st, Z(2, dtype=u8), Z()))
row("remd_loss_backward-branch-dtype", lambda: ops.remd_loss_backward(RX, RY, _remd_state(), Z(2, dtype=i32), Z()))
row("remd_loss_backward-branch-count", lambda: ops.remd_loss_backward(RX, RY, _remd_state(), Z(3, dtype=u8), Z()))
row("remd_loss_backward-branch-not-a-tensor", lambda: ops.remd_loss_backward(RX, RY, _remd_state(), None, Z()))
row("remd_loss_backward-grad-dtype", lambda: ops.remd_loss_backward(RX, RY, _remd_state(), Z(2, dtype=u8),
                                                                    Z(dtype=torch.float64)))
row("remd_loss_backward-grad-not-scalar", lambda: ops.remd_loss_backward(RX, RY, _remd_state(), Z(2, dtype=u8), Z(2)))
row("remd_loss_backward-grad-not-a-tensor", lambda: ops.remd_loss_backward(RX, RY, _remd_state(), Z(2, dtype=u8), 1.0))
row("remd_loss_backward-pair", lambda: ops.remd_loss_backward(RX, Z(1, 4, 2, 3), _remd_state(), Z(2, dtype=u8), Z()))

SS_STATE = {"inv_x": ((2, 2, 2), f32), "inv_c": ((2, 2, 2), f32), "r_x": ((2, 2, 2), f32), "r_c": ((2, 2, 2), f32),
            "t": ((2, 2, 2), f32), "pos": ((2, 4, 1), i64), "neg": ((2, 4, 1), i64)}
_ss_state = _state_rows("selfsim_loss_backward", SS_STATE, ["inv_x", "r_x", "t", "pos", "neg"],
                        lambda st: ops.selfsim_loss_backward(RX, st, Z()))
row("selfsim_loss_backward-grad-dtype", lambda: ops.selfsim_loss_backward(RX, _ss_state(), Z(dtype=torch.float64)))
row("selfsim_loss_backward-grad-not-scalar", lambda: ops.selfsim_loss_backward(RX, _ss_state(), Z(2)))
row("selfsim_loss_backward-grad-not-a-tensor", lambda: ops.selfsim_loss_backward(RX, _ss_state(), 1.0))
row("selfsim_loss_backward-pixels", lambda: ops.selfsim_loss_backward(M(1, 2, 129, 128), _ss_state(), Z()))

CX_STATE = {"xc": ((2, 3, 2, 2), f32), "yc": ((1, 3, 2, 3), f32), "inv_x": ((2, 2, 2), f32), "inv_y": ((1, 2, 3), f32),
            "row_min": ((2, 2, 2), f32), "row_index": ((2, 2, 2), i32), "row_sum": ((2, 2, 2), f32),
            "row_dsum": ((2, 2, 2), f32), "col_cx": ((2, 2, 3), f32), "col_index": ((2, 2, 3), i32),
            "col_dist": ((2, 2, 3), f32), "per_sample_cx": ((2,), f32)}
_cx_state = _state_rows("cx_loss_backward", CX_STATE, [k for k in CX_STATE if k != "col_cx"],
                        lambda st: ops.cx_loss_backward(RX, RY, st, Z()))
row("cx_loss_backward-grad-dtype", lambda: ops.cx_loss_backward(RX, RY, _cx_state(), Z(dtype=torch.float64)))
row("cx_loss_backward-grad-not-scalar", lambda: ops.cx_loss_backward(RX, RY, _cx_state(), Z(2)))
row("cx_loss_backward-grad-not-a-tensor", lambda: ops.cx_loss_backward(RX, RY, _cx_state(), 1.0))
row("cx_loss_backward-h", lambda: ops.cx_loss_backward(RX, RY, _cx_state(), Z(), h=0.0))
row("cx_loss_backward-xc-alone-empty", lambda: ops.cx_loss_backward(RX, RY, _cx_state(xc=Z(0)), Z()))

MO_STATE = {"mean_x": ((2, 3), f32), "sign_mu": ((2, 3), i8), "sign_cov": ((2, 3, 3), i8), "sums": ((2,), f32)}
_mo_state = _state_rows("moment_loss_backward", MO_STATE, ["mean_x", "sign_mu", "sign_cov"],
                        lambda st: ops.moment_loss_backward(RX, st, Z()), other=i8, exact=False)   # the first three
row("moment_loss_backward-state-two", lambda: ops.moment_loss_backward(RX, _mo_state()[:2], Z()))
row("moment_loss_backward-grad-dtype", lambda: ops.moment_loss_backward(RX, _mo_state(), Z(dtype=torch.float64)))
row("moment_loss_backward-grad-not-scalar", lambda: ops.moment_loss_backward(RX, _mo_state(), Z(2)))
row("moment_loss_backward-grad-not-a-tensor", lambda: ops.moment_loss_backward(RX, _mo_state(), 1.0))
row("moment_loss_backward-out-strided", lambda: ops.moment_loss_backward(RX, _mo_state(), Z(),
                                                                         out=Z(2, 3, 2, 4)[..., ::2]))
row("moment_loss_backward-out-shape", lambda: ops.moment_loss_backward(RX, _mo_state(), Z(), out=Z(2, 3, 2, 3)))
row("moment_loss_backward-out-dtype", lambda: ops.moment_loss_backward(RX, _mo_state(), Z(),
                                                                       out=Z(2, 3, 2, 2, dtype=torch.float64)))
row("moment_loss_backward-out-not-a-tensor", lambda: ops.moment_loss_backward(RX, _mo_state(), Z(), out=[0.0]))
row("moment_loss_backward-one-pixel", lambda: ops.moment_loss_backward(Z(2, 3, 1, 1), _mo_state(), Z()))

# the index of both gathers
for _name, _op in (("patch_gather", ops.patch_gather), ("patch_gather_guided", ops.patch_gather_guided)):
    row(f"{_name}-index-dtype", lambda op=_op: op(A, Z(2, 3, 4, dtype=i64), A))
    row(f"{_name}-index-shape", lambda op=_op: op(A, Z(2, 5, 6, dtype=i32), A))
    row(f"{_name}-index-not-a-tensor", lambda op=_op: op(A, None, A))

# the guided swap: the bank (no batch rule, below 2^31 patches) and the class maps
BANK_OPS = {
    "patch_match_guided": lambda a, b, cc=None, sc=None: ops.patch_match_guided(a, b, cc, sc),
    "patch_gather_guided": lambda a, b: ops.patch_gather_guided(b, Z(2, 3, 4, dtype=i32), a),
    "style_swap_guided": lambda a, b, cc=None, sc=None: ops.style_swap_guided(a, b, cc, sc),
}
for _name, _op in BANK_OPS.items():
    row(f"{_name}-rank", lambda op=_op: op(A, Z(4, 5, 6)))
    row(f"{_name}-channels", lambda op=_op: op(A, Z(3, 3, 5, 6)))
    row(f"{_name}-empty", lambda op=_op: op(A, Z(0, 4, 5, 6)))
    row(f"{_name}-side", lambda op=_op: op(A, Z(3, 4, 2, 6)))
    row(f"{_name}-side-first", lambda op=_op: op(Z(2, 4, 5, 2), A))
    row(f"{_name}-not-a-tensor", lambda op=_op: op(A, None))
    row(f"{_name}-2^31-patches", lambda op=_op: op(M(2, 1, 5, 6), M(1 << 29, 1, 4, 4)))
    if _name != "patch_gather_guided":
        row(f"{_name}-content_class-dtype", lambda op=_op: op(A, Z(3, 4, 5, 6), Z(2, 3, 4, dtype=i32)))
        row(f"{_name}-content_class-shape", lambda op=_op: op(A, Z(3, 4, 5, 6), Z(2, 5, 6, dtype=u8)))
        row(f"{_name}-content_class-not-a-tensor", lambda op=_op: op(A, Z(3, 4, 5, 6), [[0]]))
        row(f"{_name}-style_class-dtype", lambda op=_op: op(A, Z(3, 4, 5, 6), None, Z(3, 3, 4, dtype=i32)))
        row(f"{_name}-style_class-shape", lambda op=_op: op(A, Z(3, 4, 5, 6), None, Z(2, 3, 4, dtype=u8)))
row("patch_classes-dtype", lambda: ops.patch_classes(Z(2, 5, 6, dtype=i32)))
row("patch_classes-side", lambda: ops.patch_classes(Z(2, 2, 6, dtype=u8)))

# a map and its labels; a label map alone
LAB = Z(2, 5, 6, dtype=u8)
MAP_OPS = {
    "region_stats": lambda x, lab: ops.region_stats(x, lab, 2),
    "adain_regions": lambda x, lab: ops.adain_regions(x, lab, Z(1, 4), Z(1, 4), Z(1, 1)),
    "wct_region_cov": lambda x, lab: ops.wct_region_cov(x, lab, 2),
    "wct_region_apply": lambda x, lab: ops.wct_region_apply(x, lab, Z(2, 1, 4), Z(2, 1, 4, 4), Z(1, 4), Z(1, 4, 4),
                                                            Z(1, 1)),
    "wct_regions": lambda x, lab: ops.wct_regions(x, lab, Z(1, 4, 3, 3), Z(1, 1)),
    "efdm_region_sort": lambda x, lab: ops.efdm_region_sort(x, lab, 2),
    "efdm_regions": lambda x, lab: ops.efdm_regions(x, lab, Z(1, 4, 3, 3), Z(1, 1)),
    "kmeans_update": lambda x, lab: ops.kmeans_update(x, lab, Z(2, 4)),
}
for _name, _op in MAP_OPS.items():
    row(f"{_name}-labels-int32", lambda op=_op: op(A, LAB.int()))
    row(f"{_name}-labels-int32-before-the-map", lambda op=_op: op(Z(4, 5, 6, dtype=torch.float64), LAB.int()))
    row(f"{_name}-labels-rank", lambda op=_op: op(A, Z(5, 6, dtype=u8)))
    row(f"{_name}-labels-shape", lambda op=_op: op(A, Z(2, 6, 5, dtype=u8)))
    row(f"{_name}-map-rank", lambda op=_op: op(Z(4, 5, 6), LAB))
row("region_stats-labels-not-a-tensor", lambda: ops.region_stats(A, [[0]], 2))
row("region_stats-labels-empty", lambda: ops.region_stats(A, Z(2, 0, 6, dtype=u8), 2))
row("region_stats-map-empty", lambda: ops.region_stats(Z(2, 0, 5, 6), LAB, 2))
row("region_stats-map-not-a-tensor", lambda: ops.region_stats(None, LAB, 2))
row("region_stats-map-before-labels", lambda: ops.region_stats(None, [[0]], 2))
for _name, _op in (("resize_labels", lambda lab: ops.resize_labels(lab, 3, 3)),
                   ("label_mode_filter", lambda lab: ops.label_mode_filter(lab, 2))):
    row(f"{_name}-int32", lambda op=_op: op(LAB.int()))
    row(f"{_name}-rank", lambda op=_op: op(Z(5, 6, dtype=u8)))
    row(f"{_name}-empty", lambda op=_op: op(Z(2, 0, 6, dtype=u8)))
    row(f"{_name}-not-a-tensor", lambda op=_op: op([[0]]))
row("efdm_region_sort-no-labels-rank", lambda: ops.efdm_region_sort(Z(4, 5, 6), None, 2))

# the style bank of the regional transforms, their mix and the bank's own labels
for _name, _op in (("wct_regions", ops.wct_regions), ("efdm_regions", ops.efdm_regions)):
    row(f"{_name}-bank-rank", lambda op=_op: op(A, LAB, Z(4, 3, 3), Z(1, 1)))
    row(f"{_name}-bank-channels", lambda op=_op: op(A, LAB, Z(1, 3, 3, 3), Z(1, 1)))
    row(f"{_name}-bank-empty", lambda op=_op: op(A, LAB, Z(0, 4, 3, 3), Z(1, 1)))
    row(f"{_name}-bank-not-a-tensor", lambda op=_op: op(A, LAB, None, Z(1, 1)))
    row(f"{_name}-mix-styles", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(2, 2)))
    row(f"{_name}-mix-regions", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(9, 3)))
    row(f"{_name}-mix-no-region", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(0, 3)))
    row(f"{_name}-mix-batch", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(3, 2, 3)))
    row(f"{_name}-mix-rank", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(1, 1, 2, 3)))
    row(f"{_name}-mix-dtype", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(2, 3, dtype=torch.float64)))
    row(f"{_name}-style_labels-int32", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(2, 3), Z(3, 3, 3, dtype=i32)))
    row(f"{_name}-style_labels-rank", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(2, 3), Z(3, 3, dtype=u8)))
    row(f"{_name}-style_labels-count", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(2, 3), Z(2, 3, 3, dtype=u8)))
    row(f"{_name}-style_labels-size", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(2, 3), Z(3, 5, 6, dtype=u8)))
    row(f"{_name}-style_labels-not-a-tensor", lambda op=_op: op(A, LAB, Z(3, 4, 3, 3), Z(2, 3), [[0]]))
row("wct_region_apply-mix-styles", lambda: ops.wct_region_apply(A, LAB, Z(2, 1, 4), Z(2, 1, 4, 4), Z(1, 4), Z(1, 4, 4),
                                                                Z(1, 2)))
row("wct_region_apply-mix-regions", lambda: ops.wct_region_apply(A, LAB, Z(2, 9, 4), Z(2, 9, 4, 4), Z(1, 4),
                                                                 Z(1, 4, 4), Z(9, 1)))

EXPECT = {
    'efdm-rank': (HipOpError,
        'EFDM needs non-empty NCHW maps with equal C and a style batch of N or 1: (2, 4, 5, 6) vs (4, 5, 6)'),
    'efdm-channels': (HipOpError,
        'EFDM needs non-empty NCHW maps with equal C and a style batch of N or 1: (2, 4, 5, 6) vs (2, 3, 5, 6)'),
    'efdm-batch': (HipOpError,
        'EFDM needs non-empty NCHW maps with equal C and a style batch of N or 1: (3, 4, 5, 6) vs (2, 4, 5, 6)'),
    'efdm-empty': (HipOpError,
        'EFDM needs non-empty NCHW maps with equal C and a style batch of N or 1: (2, 4, 5, 6) vs (2, 4, 0, 6)'),
    'wct-rank': (HipOpError,
        'WCT needs non-empty NCHW maps with equal C and a style batch of N or 1: (2, 4, 5, 6) vs (4, 5, 6)'),
    'wct-channels': (HipOpError,
        'WCT needs non-empty NCHW maps with equal C and a style batch of N or 1: (2, 4, 5, 6) vs (2, 3, 5, 6)'),
    'wct-batch': (HipOpError,
        'WCT needs non-empty NCHW maps with equal C and a style batch of N or 1: (3, 4, 5, 6) vs (2, 4, 5, 6)'),
    'wct-empty': (HipOpError,
        'WCT needs non-empty NCHW maps with equal C and a style batch of N or 1: (2, 4, 5, 6) vs (2, 4, 0, 6)'),
    'patch_match-rank': (HipOpError,
        'patch_match needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_key (2, 4, 5, 6) vs style_key (4, 5, 6)'),
    'patch_match-channels': (HipOpError,
        'patch_match needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_key (2, 4, 5, 6) vs style_key (2, 3, 5, 6)'),
    'patch_match-batch': (HipOpError,
        'patch_match needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_key (3, 4, 5, 6) vs style_key (2, 4, 5, 6)'),
    'patch_match-empty': (HipOpError,
        'patch_match needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_key (2, 4, 5, 6) vs style_key (2, 4, 0, 6)'),
    'patch_match-side': (HipOpError,
        'patch_match needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_key (2, 4, 5, 6) vs style_key (2, 4, 2, 6)'),
    'patch_match-side-first': (HipOpError,
        'patch_match needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_key (2, 4, 5, 2) vs style_key (2, 4, 5, 6)'),
    'patch_gather-rank': (HipOpError,
        'patch_gather needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 6) vs style_value (4, 5, 6)'),
    'patch_gather-channels': (HipOpError,
        'patch_gather needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 6) vs style_value (2, 3, 5, 6)'),
    'patch_gather-batch': (HipOpError,
        'patch_gather needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (3, 4, 5, 6) vs style_value (2, 4, 5, 6)'),
    'patch_gather-empty': (HipOpError,
        'patch_gather needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 6) vs style_value (2, 4, 0, 6)'),
    'patch_gather-side': (HipOpError,
        'patch_gather needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 6) vs style_value (2, 4, 2, 6)'),
    'patch_gather-side-first': (HipOpError,
        'patch_gather needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 2) vs style_value (2, 4, 5, 6)'),
    'style_swap-rank': (HipOpError,
        'style_swap needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 6) vs style_map (4, 5, 6)'),
    'style_swap-channels': (HipOpError,
        'style_swap needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 6) vs style_map (2, 3, 5, 6)'),
    'style_swap-batch': (HipOpError,
        'style_swap needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (3, 4, 5, 6) vs style_map (2, 4, 5, 6)'),
    'style_swap-empty': (HipOpError,
        'style_swap needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 6) vs style_map (2, 4, 0, 6)'),
    'style_swap-side': (HipOpError,
        'style_swap needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 6) vs style_map (2, 4, 2, 6)'),
    'style_swap-side-first': (HipOpError,
        'style_swap needs non-empty NCHW maps with equal C, sides of at least 3 and a style batch of N or 1: '
        'content_map (2, 4, 5, 2) vs style_map (2, 4, 5, 6)'),
    'cosine_match-rank': (HipOpError,
        'cosine_match needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (4, 5, 6)'),
    'cosine_match-channels': (HipOpError,
        'cosine_match needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (2, 3, 5, '
        '6)'),
    'cosine_match-batch': (HipOpError,
        'cosine_match needs non-empty NCHW maps with equal C and a style batch of N or 1: x (3, 4, 5, 6) vs y (2, 4, 5, '
        '6)'),
    'cosine_match-empty': (HipOpError,
        'cosine_match needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (2, 4, 0, '
        '6)'),
    'remd_loss-rank': (HipOpError,
        'remd_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (4, 5, 6)'),
    'remd_loss-channels': (HipOpError,
        'remd_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (2, 3, 5, 6)'),
    'remd_loss-batch': (HipOpError,
        'remd_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (3, 4, 5, 6) vs y (2, 4, 5, 6)'),
    'remd_loss-empty': (HipOpError,
        'remd_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (2, 4, 0, 6)'),
    'selfsim_loss-rank': (HipOpError,
        'selfsim_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (4, 5, 6)'),
    'selfsim_loss-channels': (HipOpError,
        'selfsim_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (2, 3, 5, '
        '6)'),
    'selfsim_loss-batch': (HipOpError,
        'selfsim_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (3, 4, 5, 6) vs y (2, 4, 5, '
        '6)'),
    'selfsim_loss-empty': (HipOpError,
        'selfsim_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (2, 4, 0, '
        '6)'),
    'cx_loss-rank': (HipOpError,
        'cx_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (4, 5, 6)'),
    'cx_loss-channels': (HipOpError,
        'cx_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (2, 3, 5, 6)'),
    'cx_loss-batch': (HipOpError,
        'cx_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (3, 4, 5, 6) vs y (2, 4, 5, 6)'),
    'cx_loss-empty': (HipOpError,
        'cx_loss needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 4, 5, 6) vs y (2, 4, 0, 6)'),
    'efdm-rank-first': (HipOpError,
        'EFDM needs non-empty NCHW maps with equal C and a style batch of N or 1: (4, 5, 6) vs (2, 4, 5, 6)'),
    'efdm-empty-first': (HipOpError,
        'EFDM needs non-empty NCHW maps with equal C and a style batch of N or 1: (2, 4, 5, 0) vs (2, 4, 5, 6)'),
    'efdm-not-a-tensor': (TypeError, 'style_map must be a tensor'),
    'efdm-first-not-a-tensor': (TypeError, 'content_map must be a tensor'),
    'cosine_match-remd-channels': (HipOpError,
        'cosine_match: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 1025, 2, 2) '
        'vs y (1, 1025, 2, 2)'),
    'cosine_match-remd-pixels': (HipOpError,
        'cosine_match: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 2, 2049, '
        '2048) vs y (1, 2, 2049, 2048)'),
    'cosine_match-remd-pixels-second': (HipOpError,
        'cosine_match: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 2, 2, 2) vs '
        'y (1, 2, 2049, 2048)'),
    'cosine_match-remd-batch': (HipOpError,
        'cosine_match: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (65536, 2, 2, '
        '2) vs y (1, 2, 2, 2)'),
    'remd_loss-remd-channels': (HipOpError,
        'remd_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 1025, 2, 2) vs '
        'y (1, 1025, 2, 2)'),
    'remd_loss-remd-pixels': (HipOpError,
        'remd_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 2, 2049, 2048) '
        'vs y (1, 2, 2049, 2048)'),
    'remd_loss-remd-pixels-second': (HipOpError,
        'remd_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 2, 2, 2) vs y '
        '(1, 2, 2049, 2048)'),
    'remd_loss-remd-batch': (HipOpError,
        'remd_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (65536, 2, 2, 2) '
        'vs y (1, 2, 2, 2)'),
    'selfsim_loss-remd-channels': (HipOpError,
        'selfsim_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 1025, 2, 2) '
        'vs y (1, 1025, 2, 2)'),
    'selfsim_loss-remd-pixels': (HipOpError,
        'selfsim_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 2, 2049, '
        '2048) vs y (1, 2, 2049, 2048)'),
    'selfsim_loss-remd-pixels-second': (HipOpError,
        'selfsim_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 2, 2, 2) vs '
        'y (1, 2, 2049, 2048)'),
    'selfsim_loss-remd-batch': (HipOpError,
        'selfsim_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (65536, 2, 2, '
        '2) vs y (1, 2, 2, 2)'),
    'cx_loss-remd-channels': (HipOpError,
        'cx_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 1025, 2, 2) vs y '
        '(1, 1025, 2, 2)'),
    'cx_loss-remd-pixels': (HipOpError,
        'cx_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 2, 2049, 2048) '
        'vs y (1, 2, 2049, 2048)'),
    'cx_loss-remd-pixels-second': (HipOpError,
        'cx_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (1, 2, 2, 2) vs y '
        '(1, 2, 2049, 2048)'),
    'cx_loss-remd-batch': (HipOpError,
        'cx_loss: C is at most 1024, a map has at most 4194304 pixels and a batch 65535 samples: x (65536, 2, 2, 2) vs '
        'y (1, 2, 2, 2)'),
    'remd_loss-branch': (HipOpError, 'remd_loss: _branch is 0, 1 or 2, got 3'),
    'selfsim_loss-shapes': (HipOpError, 'selfsim_loss needs maps of equal shape: x (2, 4, 5, 6) vs c (2, 4, 6, 5)'),
    'selfsim_loss-shapes-batch': (HipOpError, 'selfsim_loss needs maps of equal shape: x (2, 4, 5, 6) vs c (1, 4, 5, 6)'),
    'selfsim_loss-pixels': (HipOpError, 'selfsim_loss: a map has at most 16384 pixels, got (1, 2, 129, 128)'),
    'selfsim_colsum-pixels': (HipOpError, 'selfsim_colsum: a map has at most 16384 pixels, got (1, 2, 129, 128)'),
    'selfsim_colsum-inv_norm': (HipOpError, 'selfsim_colsum: inv_norm must be a torch.float32 tensor (2, 5, 6) on cpu'),
    'selfsim_pairs-r_x': (HipOpError, 'selfsim_pairs: r_x must be a torch.float32 tensor (2, 5, 6) on cpu'),
    'cx_loss-pixels': (HipOpError,
        'cx_loss: C is at most 1024 and a map has at most 16384 pixels: x (1, 2, 129, 128) vs y (1, 2, 2, 2)'),
    'cx_loss-pixels-second': (HipOpError,
        'cx_loss: C is at most 1024 and a map has at most 16384 pixels: x (1, 2, 2, 2) vs y (1, 2, 129, 128)'),
    'cx_loss-h-zero': (HipOpError, 'cx_loss: the bandwidth h must be positive and finite, got 0.0'),
    'cx_loss-h-negative': (HipOpError, 'cx_loss: the bandwidth h must be positive and finite, got -0.5'),
    'cx_loss-h-inf': (HipOpError, 'cx_loss: the bandwidth h must be positive and finite, got inf'),
    'cx_loss-h-nan': (HipOpError, 'cx_loss: the bandwidth h must be positive and finite, got nan'),
    'cx_center-pixels': (HipOpError,
        'cx_center: C is at most 1024 and a map has at most 16384 pixels: x (1, 2, 129, 128) vs y (1, 2, 2, 2)'),
    'cx_rowsum-h': (HipOpError, 'cx_rowsum: the bandwidth h must be positive and finite, got 0.0'),
    'cx_rowsum-inv_y': (HipOpError, 'cx_rowsum: inv_y must be a torch.float32 tensor of 60 elements on cpu'),
    'cx_colmax-row_sum': (HipOpError, 'cx_colmax: row_sum must be a torch.float32 tensor of 60 elements on cpu'),
    'moment_loss-rank': (HipOpError, 'moment_loss needs a non-empty NCHW map, got x (3, 2, 2)'),
    'moment_loss-empty': (HipOpError, 'moment_loss needs a non-empty NCHW map, got x (2, 3, 0, 2)'),
    'moment_loss-channels': (HipOpError,
        'moment_loss: C is at most 1024, a map has at least 2 pixels and a batch at most 32767 samples: x (1, 1025, 2, '
        '2)'),
    'moment_loss-one-pixel': (HipOpError,
        'moment_loss: C is at most 1024, a map has at least 2 pixels and a batch at most 32767 samples: x (2, 3, 1, 1)'),
    'moment_loss-samples': (HipOpError,
        'moment_loss: C is at most 1024, a map has at least 2 pixels and a batch at most 32767 samples: x (32768, 2, 2, '
        '2)'),
    'moment_loss-y_mean-batch': (HipOpError, 'moment_loss: y_mean must be [N or 1, 3], got (3, 3)'),
    'moment_loss-y_mean-rank': (HipOpError, 'moment_loss: y_mean must be [N or 1, 3], got (3,)'),
    'moment_loss-y_mean-not-a-tensor': (HipOpError, 'moment_loss: y_mean must be [N or 1, 3], got None'),
    'moment_loss-y_mean-channels': (HipOpError, 'moment_loss: y_mean must be a torch.float32 tensor (1, 3) on cpu'),
    'moment_loss-y_mean-dtype': (HipOpError, 'moment_loss: y_mean must be a torch.float32 tensor (2, 3) on cpu'),
    'moment_loss-y_cov-shape': (HipOpError, 'moment_loss: y_cov must be a torch.float32 tensor (2, 3, 3) on cpu'),
    'moment_loss-y_cov-dtype': (HipOpError, 'moment_loss: y_cov must be a torch.float32 tensor (2, 3, 3) on cpu'),
    'moment_loss-y_cov-not-a-tensor': (HipOpError, 'moment_loss: y_cov must be a torch.float32 tensor (2, 3, 3) on cpu'),
    'moment_stats-one-pixel': (HipOpError,
        'moment_stats: C is at most 1024, a map has at least 2 pixels and a batch at most 32767 samples: y (2, 3, 1, 1)'),
    'remd_loss_backward-inv_x-dtype': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-inv_x-shape': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-inv_y-dtype': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-inv_y-shape': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-row_min-dtype': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-row_min-shape': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-row_index-dtype': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-row_index-shape': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-col_min-dtype': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-col_min-shape': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-col_index-dtype': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-col_index-shape': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-state-short': (ValueError, 'not enough values to unpack (expected 6, got 5)'),
    'remd_loss_backward-state-long': (ValueError, 'too many values to unpack (expected 6)'),
    'remd_loss_backward-state-element-not-a-tensor': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-state-not-a-tuple': (TypeError, 'cannot unpack non-iterable NoneType object'),
    'remd_loss_backward-branch-dtype': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-branch-count': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-branch-not-a-tensor': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-grad-dtype': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-grad-not-scalar': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-grad-not-a-tensor': (HipOpError,
        "remd_loss_backward needs the state and branch of remd_loss on x's shapes and a float32 device scalar grad"),
    'remd_loss_backward-pair': (HipOpError,
        'remd_loss_backward needs non-empty NCHW maps with equal C and a style batch of N or 1: x (2, 3, 2, 2) vs y (1, '
        '4, 2, 3)'),
    'selfsim_loss_backward-inv_x-dtype': (HipOpError,
        'selfsim_loss_backward: inv_x must be a torch.float32 tensor (2, 2, 2) on cpu'),
    'selfsim_loss_backward-inv_x-shape': (HipOpError,
        'selfsim_loss_backward: inv_x must be a torch.float32 tensor (2, 2, 2) on cpu'),
    'selfsim_loss_backward-r_x-dtype': (HipOpError,
        'selfsim_loss_backward: r_x must be a torch.float32 tensor (2, 2, 2) on cpu'),
    'selfsim_loss_backward-r_x-shape': (HipOpError,
        'selfsim_loss_backward: r_x must be a torch.float32 tensor (2, 2, 2) on cpu'),
    'selfsim_loss_backward-t-dtype': (HipOpError,
        'selfsim_loss_backward: t must be a torch.float32 tensor (2, 2, 2) on cpu'),
    'selfsim_loss_backward-t-shape': (HipOpError,
        'selfsim_loss_backward: t must be a torch.float32 tensor (2, 2, 2) on cpu'),
    'selfsim_loss_backward-pos-dtype': (HipOpError,
        'selfsim_loss_backward: pos must be a torch.int64 tensor (2, 4, 1) on cpu'),
    'selfsim_loss_backward-pos-shape': (HipOpError,
        'selfsim_loss_backward: pos must be a torch.int64 tensor (2, 4, 1) on cpu'),
    'selfsim_loss_backward-neg-dtype': (HipOpError,
        'selfsim_loss_backward: neg must be a torch.int64 tensor (2, 4, 1) on cpu'),
    'selfsim_loss_backward-neg-shape': (HipOpError,
        'selfsim_loss_backward: neg must be a torch.int64 tensor (2, 4, 1) on cpu'),
    'selfsim_loss_backward-state-short': (HipOpError,
        'selfsim_loss_backward needs the state (inv_x, inv_c, r_x, r_c, t, pos, neg) of selfsim_loss'),
    'selfsim_loss_backward-state-long': (HipOpError,
        'selfsim_loss_backward needs the state (inv_x, inv_c, r_x, r_c, t, pos, neg) of selfsim_loss'),
    'selfsim_loss_backward-state-element-not-a-tensor': (HipOpError,
        'selfsim_loss_backward: inv_x must be a torch.float32 tensor (2, 2, 2) on cpu'),
    'selfsim_loss_backward-state-not-a-tuple': (HipOpError,
        'selfsim_loss_backward needs the state (inv_x, inv_c, r_x, r_c, t, pos, neg) of selfsim_loss'),
    'selfsim_loss_backward-grad-dtype': (HipOpError, 'selfsim_loss_backward needs a float32 device scalar grad'),
    'selfsim_loss_backward-grad-not-scalar': (HipOpError, 'selfsim_loss_backward needs a float32 device scalar grad'),
    'selfsim_loss_backward-grad-not-a-tensor': (HipOpError, 'selfsim_loss_backward needs a float32 device scalar grad'),
    'selfsim_loss_backward-pixels': (HipOpError,
        'selfsim_loss_backward: a map has at most 16384 pixels, got (1, 2, 129, 128)'),
    'cx_loss_backward-xc-dtype': (HipOpError, 'cx_loss_backward: xc must be a torch.float32 tensor of 24 elements on cpu'),
    'cx_loss_backward-xc-shape': (HipOpError, 'cx_loss_backward: xc must be a torch.float32 tensor of 24 elements on cpu'),
    'cx_loss_backward-yc-dtype': (HipOpError, 'cx_loss_backward: yc must be a torch.float32 tensor of 18 elements on cpu'),
    'cx_loss_backward-yc-shape': (HipOpError, 'cx_loss_backward: yc must be a torch.float32 tensor of 18 elements on cpu'),
    'cx_loss_backward-inv_x-dtype': (HipOpError,
        'cx_loss_backward: inv_x must be a torch.float32 tensor of 8 elements on cpu'),
    'cx_loss_backward-inv_x-shape': (HipOpError,
        'cx_loss_backward: inv_x must be a torch.float32 tensor of 8 elements on cpu'),
    'cx_loss_backward-inv_y-dtype': (HipOpError,
        'cx_loss_backward: inv_y must be a torch.float32 tensor of 6 elements on cpu'),
    'cx_loss_backward-inv_y-shape': (HipOpError,
        'cx_loss_backward: inv_y must be a torch.float32 tensor of 6 elements on cpu'),
    'cx_loss_backward-row_min-dtype': (HipOpError,
        'cx_loss_backward: row_min must be a torch.float32 tensor of 8 elements on cpu'),
    'cx_loss_backward-row_min-shape': (HipOpError,
        'cx_loss_backward: row_min must be a torch.float32 tensor of 8 elements on cpu'),
    'cx_loss_backward-row_index-dtype': (HipOpError,
        'cx_loss_backward: row_index must be a torch.int32 tensor of 8 elements on cpu'),
    'cx_loss_backward-row_index-shape': (HipOpError,
        'cx_loss_backward: row_index must be a torch.int32 tensor of 8 elements on cpu'),
    'cx_loss_backward-row_sum-dtype': (HipOpError,
        'cx_loss_backward: row_sum must be a torch.float32 tensor of 8 elements on cpu'),
    'cx_loss_backward-row_sum-shape': (HipOpError,
        'cx_loss_backward: row_sum must be a torch.float32 tensor of 8 elements on cpu'),
    'cx_loss_backward-row_dsum-dtype': (HipOpError,
        'cx_loss_backward: row_dsum must be a torch.float32 tensor of 8 elements on cpu'),
    'cx_loss_backward-row_dsum-shape': (HipOpError,
        'cx_loss_backward: row_dsum must be a torch.float32 tensor of 8 elements on cpu'),
    'cx_loss_backward-col_index-dtype': (HipOpError,
        'cx_loss_backward: col_index must be a torch.int32 tensor of 12 elements on cpu'),
    'cx_loss_backward-col_index-shape': (HipOpError,
        'cx_loss_backward: col_index must be a torch.int32 tensor of 12 elements on cpu'),
    'cx_loss_backward-col_dist-dtype': (HipOpError,
        'cx_loss_backward: col_dist must be a torch.float32 tensor of 12 elements on cpu'),
    'cx_loss_backward-col_dist-shape': (HipOpError,
        'cx_loss_backward: col_dist must be a torch.float32 tensor of 12 elements on cpu'),
    'cx_loss_backward-per_sample_cx-dtype': (HipOpError,
        'cx_loss_backward: per_sample_cx must be a torch.float32 tensor of 2 elements on cpu'),
    'cx_loss_backward-per_sample_cx-shape': (HipOpError,
        'cx_loss_backward: per_sample_cx must be a torch.float32 tensor of 2 elements on cpu'),
    'cx_loss_backward-state-short': (HipOpError, 'cx_loss_backward needs the state of cx_loss (12 tensors)'),
    'cx_loss_backward-state-long': (HipOpError, 'cx_loss_backward needs the state of cx_loss (12 tensors)'),
    'cx_loss_backward-state-element-not-a-tensor': (HipOpError,
        'cx_loss_backward: xc must be a torch.float32 tensor of 24 elements on cpu'),
    'cx_loss_backward-state-not-a-tuple': (HipOpError, 'cx_loss_backward needs the state of cx_loss (12 tensors)'),
    'cx_loss_backward-grad-dtype': (HipOpError,
        'cx_loss_backward: grad must be a torch.float32 tensor of 1 elements on cpu'),
    'cx_loss_backward-grad-not-scalar': (HipOpError,
        'cx_loss_backward: grad must be a torch.float32 tensor of 1 elements on cpu'),
    'cx_loss_backward-grad-not-a-tensor': (HipOpError,
        'cx_loss_backward: grad must be a torch.float32 tensor of 1 elements on cpu'),
    'cx_loss_backward-h': (HipOpError, 'cx_loss_backward: the bandwidth h must be positive and finite, got 0.0'),
    'cx_loss_backward-xc-alone-empty': (HipOpError,
        'cx_loss_backward: xc must be a torch.float32 tensor of 24 elements on cpu'),
    'moment_loss_backward-mean_x-dtype': (HipOpError,
        'moment_loss_backward: mean_x must be a torch.float32 tensor (2, 3) on cpu'),
    'moment_loss_backward-mean_x-shape': (HipOpError,
        'moment_loss_backward: mean_x must be a torch.float32 tensor (2, 3) on cpu'),
    'moment_loss_backward-sign_mu-dtype': (HipOpError,
        'moment_loss_backward: sign_mu must be a torch.int8 tensor (2, 3) on cpu'),
    'moment_loss_backward-sign_mu-shape': (HipOpError,
        'moment_loss_backward: sign_mu must be a torch.int8 tensor (2, 3) on cpu'),
    'moment_loss_backward-sign_cov-dtype': (HipOpError,
        'moment_loss_backward: sign_cov must be a torch.int8 tensor (2, 3, 3) on cpu'),
    'moment_loss_backward-sign_cov-shape': (HipOpError,
        'moment_loss_backward: sign_cov must be a torch.int8 tensor (2, 3, 3) on cpu'),
    'moment_loss_backward-state-element-not-a-tensor': (HipOpError,
        'moment_loss_backward: mean_x must be a torch.float32 tensor (2, 3) on cpu'),
    'moment_loss_backward-state-not-a-tuple': (HipOpError, 'moment_loss_backward needs the state of moment_loss'),
    'moment_loss_backward-state-two': (HipOpError, 'moment_loss_backward needs the state of moment_loss'),
    'moment_loss_backward-grad-dtype': (HipOpError, 'moment_loss_backward: grad must be a torch.float32 tensor () on cpu'),
    'moment_loss_backward-grad-not-scalar': (HipOpError,
        'moment_loss_backward: grad must be a torch.float32 tensor () on cpu'),
    'moment_loss_backward-grad-not-a-tensor': (HipOpError,
        'moment_loss_backward: grad must be a torch.float32 tensor () on cpu'),
    'moment_loss_backward-out-strided': (HipOpError, 'moment_loss_backward: out must be a contiguous tensor'),
    'moment_loss_backward-out-shape': (HipOpError,
        'moment_loss_backward: out must be a torch.float32 tensor (2, 3, 2, 2) on cpu'),
    'moment_loss_backward-out-dtype': (HipOpError,
        'moment_loss_backward: out must be a torch.float32 tensor (2, 3, 2, 2) on cpu'),
    'moment_loss_backward-out-not-a-tensor': (HipOpError, 'moment_loss_backward: out must be a contiguous tensor'),
    'moment_loss_backward-one-pixel': (HipOpError,
        'moment_loss_backward: C is at most 1024, a map has at least 2 pixels and a batch at most 32767 samples: x (2, '
        '3, 1, 1)'),
    'patch_gather-index-dtype': (HipOpError, 'index must be an int32 tensor (2, 3, 4) on cpu'),
    'patch_gather-index-shape': (HipOpError, 'index must be an int32 tensor (2, 3, 4) on cpu'),
    'patch_gather-index-not-a-tensor': (HipOpError, 'index must be an int32 tensor (2, 3, 4) on cpu'),
    'patch_gather_guided-index-dtype': (HipOpError, 'index must be an int32 tensor (2, 3, 4) on cpu'),
    'patch_gather_guided-index-shape': (HipOpError, 'index must be an int32 tensor (2, 3, 4) on cpu'),
    'patch_gather_guided-index-not-a-tensor': (HipOpError, 'index must be an int32 tensor (2, 3, 4) on cpu'),
    'patch_match_guided-rank': (HipOpError,
        'patch_match_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_key (2, 4, 5, 6) vs '
        'style_keys (4, 5, 6)'),
    'patch_match_guided-channels': (HipOpError,
        'patch_match_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_key (2, 4, 5, 6) vs '
        'style_keys (3, 3, 5, 6)'),
    'patch_match_guided-empty': (HipOpError,
        'patch_match_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_key (2, 4, 5, 6) vs '
        'style_keys (0, 4, 5, 6)'),
    'patch_match_guided-side': (HipOpError,
        'patch_match_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_key (2, 4, 5, 6) vs '
        'style_keys (3, 4, 2, 6)'),
    'patch_match_guided-side-first': (HipOpError,
        'patch_match_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_key (2, 4, 5, 2) vs '
        'style_keys (2, 4, 5, 6)'),
    'patch_match_guided-not-a-tensor': (TypeError, 'style_keys must be a tensor'),
    'patch_match_guided-2^31-patches': (HipOpError,
        'patch_match_guided: a bank of 536870912 styles 4x4 has 2147483648 style patches, 2^31 or more'),
    'patch_match_guided-content_class-dtype': (HipOpError, 'content_class must be a uint8 tensor (2, 3, 4) on cpu'),
    'patch_match_guided-content_class-shape': (HipOpError, 'content_class must be a uint8 tensor (2, 3, 4) on cpu'),
    'patch_match_guided-content_class-not-a-tensor': (HipOpError, 'content_class must be a uint8 tensor (2, 3, 4) on cpu'),
    'patch_match_guided-style_class-dtype': (HipOpError, 'style_class must be a uint8 tensor (3, 3, 4) on cpu'),
    'patch_match_guided-style_class-shape': (HipOpError, 'style_class must be a uint8 tensor (3, 3, 4) on cpu'),
    'patch_gather_guided-rank': (HipOpError,
        'patch_gather_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 6) '
        'vs style_values (4, 5, 6)'),
    'patch_gather_guided-channels': (HipOpError,
        'patch_gather_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 6) '
        'vs style_values (3, 3, 5, 6)'),
    'patch_gather_guided-empty': (HipOpError,
        'patch_gather_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 6) '
        'vs style_values (0, 4, 5, 6)'),
    'patch_gather_guided-side': (HipOpError,
        'patch_gather_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 6) '
        'vs style_values (3, 4, 2, 6)'),
    'patch_gather_guided-side-first': (HipOpError,
        'patch_gather_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 2) '
        'vs style_values (2, 4, 5, 6)'),
    'patch_gather_guided-not-a-tensor': (TypeError, 'style_values must be a tensor'),
    'patch_gather_guided-2^31-patches': (HipOpError,
        'patch_gather_guided: a bank of 536870912 styles 4x4 has 2147483648 style patches, 2^31 or more'),
    'style_swap_guided-rank': (HipOpError,
        'style_swap_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 6) vs '
        'style_maps (4, 5, 6)'),
    'style_swap_guided-channels': (HipOpError,
        'style_swap_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 6) vs '
        'style_maps (3, 3, 5, 6)'),
    'style_swap_guided-empty': (HipOpError,
        'style_swap_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 6) vs '
        'style_maps (0, 4, 5, 6)'),
    'style_swap_guided-side': (HipOpError,
        'style_swap_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 6) vs '
        'style_maps (3, 4, 2, 6)'),
    'style_swap_guided-side-first': (HipOpError,
        'style_swap_guided needs non-empty NCHW maps with equal C and sides of at least 3: content_map (2, 4, 5, 2) vs '
        'style_maps (2, 4, 5, 6)'),
    'style_swap_guided-not-a-tensor': (TypeError, 'style_maps must be a tensor'),
    'style_swap_guided-2^31-patches': (HipOpError,
        'style_swap_guided: a bank of 536870912 styles 4x4 has 2147483648 style patches, 2^31 or more'),
    'style_swap_guided-content_class-dtype': (HipOpError, 'content_class must be a uint8 tensor (2, 3, 4) on cpu'),
    'style_swap_guided-content_class-shape': (HipOpError, 'content_class must be a uint8 tensor (2, 3, 4) on cpu'),
    'style_swap_guided-content_class-not-a-tensor': (HipOpError, 'content_class must be a uint8 tensor (2, 3, 4) on cpu'),
    'style_swap_guided-style_class-dtype': (HipOpError, 'style_class must be a uint8 tensor (3, 3, 4) on cpu'),
    'style_swap_guided-style_class-shape': (HipOpError, 'style_class must be a uint8 tensor (3, 3, 4) on cpu'),
    'patch_classes-dtype': (HipOpError, 'patch_classes needs a uint8 label map [B, h, w] with sides of at least 3'),
    'patch_classes-side': (HipOpError, 'patch_classes needs a uint8 label map [B, h, w] with sides of at least 3'),
    'region_stats-labels-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'region_stats-labels-int32-before-the-map': (HipOpError, 'labels must be uint8, got torch.int32'),
    'region_stats-labels-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'region_stats-labels-shape': (HipOpError, 'labels must be [N, H, W] = (2, 5, 6) on cpu, got (2, 6, 5) on cpu'),
    'region_stats-map-rank': (HipOpError, 'x must be a non-empty NCHW map, got (4, 5, 6)'),
    'adain_regions-labels-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'adain_regions-labels-int32-before-the-map': (HipOpError, 'labels must be uint8, got torch.int32'),
    'adain_regions-labels-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'adain_regions-labels-shape': (HipOpError, 'labels must be [N, H, W] = (2, 5, 6) on cpu, got (2, 6, 5) on cpu'),
    'adain_regions-map-rank': (HipOpError, 'content_map must be a non-empty NCHW map, got (4, 5, 6)'),
    'wct_region_cov-labels-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'wct_region_cov-labels-int32-before-the-map': (HipOpError, 'labels must be uint8, got torch.int32'),
    'wct_region_cov-labels-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'wct_region_cov-labels-shape': (HipOpError, 'labels must be [N, H, W] = (2, 5, 6) on cpu, got (2, 6, 5) on cpu'),
    'wct_region_cov-map-rank': (HipOpError, 'x must be a non-empty NCHW map, got (4, 5, 6)'),
    'wct_region_apply-labels-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'wct_region_apply-labels-int32-before-the-map': (HipOpError, 'labels must be uint8, got torch.int32'),
    'wct_region_apply-labels-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'wct_region_apply-labels-shape': (HipOpError, 'labels must be [N, H, W] = (2, 5, 6) on cpu, got (2, 6, 5) on cpu'),
    'wct_region_apply-map-rank': (HipOpError, 'content_map must be a non-empty NCHW map, got (4, 5, 6)'),
    'wct_regions-labels-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'wct_regions-labels-int32-before-the-map': (HipOpError, 'labels must be uint8, got torch.int32'),
    'wct_regions-labels-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'wct_regions-labels-shape': (HipOpError, 'labels must be [N, H, W] = (2, 5, 6) on cpu, got (2, 6, 5) on cpu'),
    'wct_regions-map-rank': (HipOpError, 'content_map must be a non-empty NCHW map, got (4, 5, 6)'),
    'efdm_region_sort-labels-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'efdm_region_sort-labels-int32-before-the-map': (HipOpError, 'labels must be uint8, got torch.int32'),
    'efdm_region_sort-labels-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'efdm_region_sort-labels-shape': (HipOpError, 'labels must be [N, H, W] = (2, 5, 6) on cpu, got (2, 6, 5) on cpu'),
    'efdm_region_sort-map-rank': (HipOpError, 'x must be a non-empty NCHW map, got (4, 5, 6)'),
    'efdm_regions-labels-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'efdm_regions-labels-int32-before-the-map': (HipOpError, 'labels must be uint8, got torch.int32'),
    'efdm_regions-labels-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'efdm_regions-labels-shape': (HipOpError, 'labels must be [N, H, W] = (2, 5, 6) on cpu, got (2, 6, 5) on cpu'),
    'efdm_regions-map-rank': (HipOpError, 'content_map must be a non-empty NCHW map, got (4, 5, 6)'),
    'kmeans_update-labels-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'kmeans_update-labels-int32-before-the-map': (HipOpError, 'labels must be uint8, got torch.int32'),
    'kmeans_update-labels-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'kmeans_update-labels-shape': (HipOpError, 'labels must be [N, H, W] = (2, 5, 6) on cpu, got (2, 6, 5) on cpu'),
    'kmeans_update-map-rank': (HipOpError, 'x must be a non-empty NCHW map, got (4, 5, 6)'),
    'region_stats-labels-not-a-tensor': (TypeError, 'labels must be a tensor'),
    'region_stats-labels-empty': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (2, 0, 6)'),
    'region_stats-map-empty': (HipOpError, 'x must be a non-empty NCHW map, got (2, 0, 5, 6)'),
    'region_stats-map-not-a-tensor': (TypeError, 'x must be a tensor'),
    'region_stats-map-before-labels': (TypeError, 'x must be a tensor'),
    'resize_labels-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'resize_labels-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'resize_labels-empty': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (2, 0, 6)'),
    'resize_labels-not-a-tensor': (TypeError, 'labels must be a tensor'),
    'label_mode_filter-int32': (HipOpError, 'labels must be uint8, got torch.int32'),
    'label_mode_filter-rank': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (5, 6)'),
    'label_mode_filter-empty': (HipOpError, 'labels must be a non-empty [N, H, W] uint8 map, got (2, 0, 6)'),
    'label_mode_filter-not-a-tensor': (TypeError, 'labels must be a tensor'),
    'efdm_region_sort-no-labels-rank': (HipOpError, 'x must be a non-empty NCHW map, got (4, 5, 6)'),
    'wct_regions-bank-rank': (HipOpError,
        'wct_regions needs a non-empty style bank [S, C=4, Hs, Ws] on cpu, got (4, 3, 3) on cpu'),
    'wct_regions-bank-channels': (HipOpError,
        'wct_regions needs a non-empty style bank [S, C=4, Hs, Ws] on cpu, got (1, 3, 3, 3) on cpu'),
    'wct_regions-bank-empty': (HipOpError,
        'wct_regions needs a non-empty style bank [S, C=4, Hs, Ws] on cpu, got (0, 4, 3, 3) on cpu'),
    'wct_regions-bank-not-a-tensor': (TypeError, 'styles must be a tensor'),
    'wct_regions-mix-styles': (HipOpError, 'wct_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (1, 2, 2) on cpu'),
    'wct_regions-mix-regions': (HipOpError,
        'wct_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (1, 9, 3) on cpu'),
    'wct_regions-mix-no-region': (HipOpError,
        'wct_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (1, 0, 3) on cpu'),
    'wct_regions-mix-batch': (HipOpError, 'wct_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (3, 2, 3) on cpu'),
    'wct_regions-mix-rank': (HipOpError,
        'wct_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (1, 1, 2, 3) on cpu'),
    'wct_regions-mix-dtype': (HipOpError, 'mix must be float32, got torch.float64'),
    'wct_regions-style_labels-int32': (HipOpError, 'style_labels must be uint8, got torch.int32'),
    'wct_regions-style_labels-rank': (HipOpError, 'style_labels must be a non-empty [N, H, W] uint8 map, got (3, 3)'),
    'wct_regions-style_labels-count': (HipOpError,
        'style_labels must be [S, Hs, Ws] = (3, 3, 3) on cpu, got (2, 3, 3) on cpu'),
    'wct_regions-style_labels-size': (HipOpError,
        'style_labels must be [S, Hs, Ws] = (3, 3, 3) on cpu, got (3, 5, 6) on cpu'),
    'wct_regions-style_labels-not-a-tensor': (TypeError, 'style_labels must be a tensor'),
    'efdm_regions-bank-rank': (HipOpError,
        'efdm_regions needs a non-empty style bank [S, C=4, Hs, Ws] on cpu, got (4, 3, 3) on cpu'),
    'efdm_regions-bank-channels': (HipOpError,
        'efdm_regions needs a non-empty style bank [S, C=4, Hs, Ws] on cpu, got (1, 3, 3, 3) on cpu'),
    'efdm_regions-bank-empty': (HipOpError,
        'efdm_regions needs a non-empty style bank [S, C=4, Hs, Ws] on cpu, got (0, 4, 3, 3) on cpu'),
    'efdm_regions-bank-not-a-tensor': (TypeError, 'styles must be a tensor'),
    'efdm_regions-mix-styles': (HipOpError,
        'efdm_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (1, 2, 2) on cpu'),
    'efdm_regions-mix-regions': (HipOpError,
        'efdm_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (1, 9, 3) on cpu'),
    'efdm_regions-mix-no-region': (HipOpError,
        'efdm_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (1, 0, 3) on cpu'),
    'efdm_regions-mix-batch': (HipOpError,
        'efdm_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (3, 2, 3) on cpu'),
    'efdm_regions-mix-rank': (HipOpError,
        'efdm_regions: mix must be [N=2 or 1, K <= 8, S=3] on cpu, got (1, 1, 2, 3) on cpu'),
    'efdm_regions-mix-dtype': (HipOpError, 'mix must be float32, got torch.float64'),
    'efdm_regions-style_labels-int32': (HipOpError, 'style_labels must be uint8, got torch.int32'),
    'efdm_regions-style_labels-rank': (HipOpError, 'style_labels must be a non-empty [N, H, W] uint8 map, got (3, 3)'),
    'efdm_regions-style_labels-count': (HipOpError,
        'style_labels must be [S, Hs, Ws] = (3, 3, 3) on cpu, got (2, 3, 3) on cpu'),
    'efdm_regions-style_labels-size': (HipOpError,
        'style_labels must be [S, Hs, Ws] = (3, 3, 3) on cpu, got (3, 5, 6) on cpu'),
    'efdm_regions-style_labels-not-a-tensor': (TypeError, 'style_labels must be a tensor'),
    'wct_region_apply-mix-styles': (HipOpError,
        'wct_region_apply: mix must be [N=2 or 1, K <= 8, S=1] on cpu, got (1, 1, 2) on cpu'),
    'wct_region_apply-mix-regions': (HipOpError,
        'wct_region_apply: mix must be [N=2 or 1, K <= 8, S=1] on cpu, got (1, 9, 1) on cpu'),
}


@pytest.mark.parametrize("rid", [r[0] for r in ROWS])
def test_invalid_op_call_raises_its_type_and_message(rid, host_only):
    kind, message = EXPECT[rid]
    with pytest.raises(kind) as e:
        dict(ROWS)[rid]()
    assert type(e.value) is kind and str(e.value) == message


# ---- the regional methods of the model ------------------------------------------------------------------

from test_efdm_regions_cpu import _Relu41Stub  # noqa: E402  (a relu4_1-shaped map of zeros in the encoder's place)

REGIONAL = ("stylize_regions", "stylize_regions_wct", "stylize_regions_efdm", "stylize_swap_regions")
WEIGHTED = REGIONAL[:3]
IMG = Z(1, 3, 32, 32)                      # relu4_1: 4 x 4
AT_IMG, AT_FEAT = Z(1, 32, 32, dtype=u8), Z(1, 4, 4, dtype=u8)
AUTO = models.AutoRegions(2)


def styles(s):
    return IMG.expand(s, -1, -1, -1)


# id -> (the methods it applies to, autograd on, call(bound method))
MODEL_ROWS = {
    "under-grad": (REGIONAL, True, lambda m: m(IMG, IMG)),
    "under-grad-preserve_color": (REGIONAL, True, lambda m: m(IMG, IMG, preserve_color=True)),
    "under-grad-bad-images": (REGIONAL, True, lambda m: m(IMG[0], IMG)),
    "content-rank": (REGIONAL, False, lambda m: m(IMG[0], IMG)),
    "style-rank": (REGIONAL, False, lambda m: m(IMG, IMG[0])),
    "auto-with-style_labels": (REGIONAL, False, lambda m: m(IMG, IMG, labels=AUTO, style_labels=AT_FEAT)),
    "auto-with-weights": (WEIGHTED, False, lambda m: m(IMG, IMG, labels=AUTO, weights=[[1.0], [1.0]])),
    "auto-before-too-many-styles": (WEIGHTED, False, lambda m: m(IMG, styles(65), labels=AUTO, weights=[[1.0]])),
    "too-many-styles": (WEIGHTED, False, lambda m: m(IMG, styles(65))),
    "too-many-styles-auto": (WEIGHTED, False, lambda m: m(IMG, styles(65), labels=AUTO)),
    "too-many-styles-for-their-regions": (WEIGHTED, False, lambda m: m(IMG, styles(9), labels=AT_FEAT)),
    "too-many-styles-before-weights": (WEIGHTED, False, lambda m: m(IMG, styles(65), weights=[[1.0, 2.0]])),
    "too-many-rows": (REGIONAL[:1], False, lambda m: m(IMG, styles(9), labels=AT_FEAT, style_labels=AT_FEAT.expand(9, -1, -1),
                                                   weights=[[1.0] * 9] * 8)),
    "too-many-rows-auto": (REGIONAL[:1], False, lambda m: m(IMG, styles(33), labels=AUTO)),
    "weights-shape": (WEIGHTED, False, lambda m: m(IMG, IMG, weights=[[1.0, 2.0]])),
    "weights-batch": (WEIGHTED, False, lambda m: m(IMG, IMG, weights=[[[1.0]], [[1.0]]])),
    "weights-regions": (WEIGHTED, False, lambda m: m(IMG, IMG, labels=AT_FEAT, weights=[[1.0]] * 9)),
    "weights-single-region": (WEIGHTED, False, lambda m: m(IMG, styles(2), weights=[[1.0, 0.0], [0.0, 1.0]])),
    "weights-zero-row": (WEIGHTED, False, lambda m: m(IMG, IMG, weights=[[0.0]])),
    "weights-negative": (WEIGHTED, False, lambda m: m(IMG, styles(2), weights=[[2.0, -1.0]])),
    "weights-nan": (WEIGHTED, False, lambda m: m(IMG, IMG, weights=[[float("nan")]])),
    "weights-not-numbers": (WEIGHTED, False, lambda m: m(IMG, IMG, weights=[["a"]])),
    "weights-on-meta": (WEIGHTED, False, lambda m: m(IMG, IMG, weights=M(1, 1))),
    "style_labels-without-labels": (REGIONAL[3:], False, lambda m: m(IMG, IMG, style_labels=AT_FEAT)),
    "too-many-styles-for-their-classes": (REGIONAL[3:], False, lambda m: m(IMG, styles(65), labels=AT_FEAT)),
    "labels-resolution": (REGIONAL, False, lambda m: m(IMG, IMG, labels=AT_IMG[:, :5, :5])),
    "labels-count": (REGIONAL, False, lambda m: m(IMG, IMG, labels=AT_IMG.expand(2, -1, -1))),
    "labels-type": (REGIONAL, False, lambda m: m(IMG, IMG, labels=[[0]])),
    "labels-rank": (REGIONAL, False, lambda m: m(IMG, IMG, labels=AT_FEAT.unsqueeze(0))),
    "style_labels-resolution": (REGIONAL, False, lambda m: m(IMG, IMG, labels=AT_FEAT, style_labels=AT_IMG[:, :7])),
    "style_labels-count": (REGIONAL, False, lambda m: m(IMG, IMG, labels=AT_FEAT, style_labels=AT_FEAT.expand(2, -1, -1))),
    "style_labels-type": (REGIONAL, False, lambda m: m(IMG, IMG, labels=AT_FEAT, style_labels=[[0]])),
    "labels-before-style_labels": (REGIONAL, False, lambda m: m(IMG, IMG, labels=[[0]], style_labels=[[0]])),
}

# the other guards of the model: (method, autograd on, call(net))
OTHER_ROWS = {
    "forward-preserve_color-under-grad": (True, lambda net: net(IMG, IMG, preserve_color=True)),
    "stylize_swap-under-grad": (True, lambda net: net.stylize_swap(IMG, IMG)),
    "stylize_with_stats-under-grad": (True, lambda net: net.stylize_with_stats(IMG, Z(512), Z(512))),
    "auto_labels-under-grad": (True, lambda net: net.auto_labels(IMG, IMG)),
    "auto_labels-auto": (False, lambda net: net.auto_labels(IMG, IMG, auto=2)),
    "auto_labels-rank": (False, lambda net: net.auto_labels(IMG[0], IMG)),
}

MODEL_EXPECT = {
    ('under-grad', 'stylize_regions'): (NotImplementedError,
        'stylize_regions is inference-only; run it under torch.no_grad()'),
    ('under-grad', 'stylize_regions_wct'): (NotImplementedError,
        'stylize_regions_wct is inference-only; run it under torch.no_grad()'),
    ('under-grad', 'stylize_regions_efdm'): (NotImplementedError,
        'stylize_regions_efdm is inference-only; run it under torch.no_grad()'),
    ('under-grad', 'stylize_swap_regions'): (NotImplementedError,
        'stylize_swap_regions is inference-only; run it under torch.no_grad()'),
    ('under-grad-preserve_color', 'stylize_regions'): (NotImplementedError,
        'stylize_regions is inference-only; run it under torch.no_grad()'),
    ('under-grad-preserve_color', 'stylize_regions_wct'): (NotImplementedError,
        'stylize_regions_wct is inference-only; run it under torch.no_grad()'),
    ('under-grad-preserve_color', 'stylize_regions_efdm'): (NotImplementedError,
        'stylize_regions_efdm is inference-only; run it under torch.no_grad()'),
    ('under-grad-preserve_color', 'stylize_swap_regions'): (NotImplementedError,
        'stylize_swap_regions is inference-only; run it under torch.no_grad()'),
    ('under-grad-bad-images', 'stylize_regions'): (NotImplementedError,
        'stylize_regions is inference-only; run it under torch.no_grad()'),
    ('under-grad-bad-images', 'stylize_regions_wct'): (NotImplementedError,
        'stylize_regions_wct is inference-only; run it under torch.no_grad()'),
    ('under-grad-bad-images', 'stylize_regions_efdm'): (NotImplementedError,
        'stylize_regions_efdm is inference-only; run it under torch.no_grad()'),
    ('under-grad-bad-images', 'stylize_swap_regions'): (NotImplementedError,
        'stylize_swap_regions is inference-only; run it under torch.no_grad()'),
    ('content-rank', 'stylize_regions'): (ValueError,
        'stylize_regions needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('content-rank', 'stylize_regions_wct'): (ValueError,
        'stylize_regions_wct needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('content-rank', 'stylize_regions_efdm'): (ValueError,
        'stylize_regions_efdm needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('content-rank', 'stylize_swap_regions'): (ValueError,
        'stylize_swap_regions needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('style-rank', 'stylize_regions'): (ValueError,
        'stylize_regions needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('style-rank', 'stylize_regions_wct'): (ValueError,
        'stylize_regions_wct needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('style-rank', 'stylize_regions_efdm'): (ValueError,
        'stylize_regions_efdm needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('style-rank', 'stylize_swap_regions'): (ValueError,
        'stylize_swap_regions needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('auto-with-style_labels', 'stylize_regions'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('auto-with-style_labels', 'stylize_regions_wct'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('auto-with-style_labels', 'stylize_regions_efdm'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('auto-with-style_labels', 'stylize_swap_regions'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('auto-with-weights', 'stylize_regions'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('auto-with-weights', 'stylize_regions_wct'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('auto-with-weights', 'stylize_regions_efdm'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('auto-before-too-many-styles', 'stylize_regions'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('auto-before-too-many-styles', 'stylize_regions_wct'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('auto-before-too-many-styles', 'stylize_regions_efdm'): (ValueError,
        'labels=AutoRegions(...) makes style_labels and weights itself: leave both None'),
    ('too-many-styles', 'stylize_regions'): (ValueError,
        'at most 64 rows of style statistics (S, or K * S with style_labels)'),
    ('too-many-styles', 'stylize_regions_wct'): (ValueError, 'at most 64 styles, got 65'),
    ('too-many-styles', 'stylize_regions_efdm'): (ValueError, 'at most 64 styles, got 65'),
    ('too-many-styles-auto', 'stylize_regions'): (ValueError,
        'at most 64 rows of style statistics (S, or K * S with style_labels)'),
    ('too-many-styles-auto', 'stylize_regions_wct'): (ValueError, 'at most 64 styles, got 65'),
    ('too-many-styles-auto', 'stylize_regions_efdm'): (ValueError, 'at most 64 styles, got 65'),
    ('too-many-styles-for-their-regions', 'stylize_regions'): (ValueError,
        'weights=None assigns style k to region k: at most 8 styles, got 9'),
    ('too-many-styles-for-their-regions', 'stylize_regions_wct'): (ValueError,
        'weights=None assigns style k to region k: at most 8 styles, got 9'),
    ('too-many-styles-for-their-regions', 'stylize_regions_efdm'): (ValueError,
        'weights=None assigns style k to region k: at most 8 styles, got 9'),
    ('too-many-styles-before-weights', 'stylize_regions'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=65, K in 1..8; got (1, 1, 2)'),
    ('too-many-styles-before-weights', 'stylize_regions_wct'): (ValueError, 'at most 64 styles, got 65'),
    ('too-many-styles-before-weights', 'stylize_regions_efdm'): (ValueError, 'at most 64 styles, got 65'),
    ('too-many-rows', 'stylize_regions'): (ValueError,
        'at most 64 rows of style statistics (S, or K * S with style_labels)'),
    ('too-many-rows-auto', 'stylize_regions'): (ValueError,
        'at most 64 rows of style statistics (S, or K * S with style_labels)'),
    ('weights-shape', 'stylize_regions'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=1, K in 1..8; got (1, 1, 2)'),
    ('weights-shape', 'stylize_regions_wct'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=1, K in 1..8; got (1, 1, 2)'),
    ('weights-shape', 'stylize_regions_efdm'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=1, K in 1..8; got (1, 1, 2)'),
    ('weights-batch', 'stylize_regions'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=1, K in 1..8; got (2, 1, 1)'),
    ('weights-batch', 'stylize_regions_wct'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=1, K in 1..8; got (2, 1, 1)'),
    ('weights-batch', 'stylize_regions_efdm'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=1, K in 1..8; got (2, 1, 1)'),
    ('weights-regions', 'stylize_regions'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=1, K in 1..8; got (1, 9, 1)'),
    ('weights-regions', 'stylize_regions_wct'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=1, K in 1..8; got (1, 9, 1)'),
    ('weights-regions', 'stylize_regions_efdm'): (ValueError,
        'weights must be [K, S] or [N, K, S] with N=1, S=1, K in 1..8; got (1, 9, 1)'),
    ('weights-single-region', 'stylize_regions'): (ValueError,
        'labels=None is a single region: weights must have K = 1, got K = 2'),
    ('weights-single-region', 'stylize_regions_wct'): (ValueError,
        'labels=None is a single region: weights must have K = 1, got K = 2'),
    ('weights-single-region', 'stylize_regions_efdm'): (ValueError,
        'labels=None is a single region: weights must have K = 1, got K = 2'),
    ('weights-zero-row', 'stylize_regions'): (ValueError, 'every row of weights must sum to more than 0'),
    ('weights-zero-row', 'stylize_regions_wct'): (ValueError, 'every row of weights must sum to more than 0'),
    ('weights-zero-row', 'stylize_regions_efdm'): (ValueError, 'every row of weights must sum to more than 0'),
    ('weights-negative', 'stylize_regions'): (ValueError, 'weights must be finite and non-negative'),
    ('weights-negative', 'stylize_regions_wct'): (ValueError, 'weights must be finite and non-negative'),
    ('weights-negative', 'stylize_regions_efdm'): (ValueError, 'weights must be finite and non-negative'),
    ('weights-nan', 'stylize_regions'): (ValueError, 'weights must be finite and non-negative'),
    ('weights-nan', 'stylize_regions_wct'): (ValueError, 'weights must be finite and non-negative'),
    ('weights-nan', 'stylize_regions_efdm'): (ValueError, 'weights must be finite and non-negative'),
    ('weights-not-numbers', 'stylize_regions'): (ValueError,
        "weights must be a [K, S] or [N, K, S] array of numbers: too many dimensions 'str'"),
    ('weights-not-numbers', 'stylize_regions_wct'): (ValueError,
        "weights must be a [K, S] or [N, K, S] array of numbers: too many dimensions 'str'"),
    ('weights-not-numbers', 'stylize_regions_efdm'): (ValueError,
        "weights must be a [K, S] or [N, K, S] array of numbers: too many dimensions 'str'"),
    ('weights-on-meta', 'stylize_regions'): (ValueError, 'weights are host-side: pass a nested sequence or a CPU tensor'),
    ('weights-on-meta', 'stylize_regions_wct'): (ValueError,
        'weights are host-side: pass a nested sequence or a CPU tensor'),
    ('weights-on-meta', 'stylize_regions_efdm'): (ValueError,
        'weights are host-side: pass a nested sequence or a CPU tensor'),
    ('style_labels-without-labels', 'stylize_swap_regions'): (ValueError,
        "style_labels without labels: give the content's label map too"),
    ('too-many-styles-for-their-classes', 'stylize_swap_regions'): (ValueError,
        'labels alone assign style k to region k: at most 64 styles, got 65'),
    ('labels-resolution', 'stylize_regions'): (ValueError,
        'labels must be at the image resolution (32, 32) or the feature resolution (4, 4), got (5, 5)'),
    ('labels-resolution', 'stylize_regions_wct'): (ValueError,
        'labels must be at the image resolution (32, 32) or the feature resolution (4, 4), got (5, 5)'),
    ('labels-resolution', 'stylize_regions_efdm'): (ValueError,
        'labels must be at the image resolution (32, 32) or the feature resolution (4, 4), got (5, 5)'),
    ('labels-resolution', 'stylize_swap_regions'): (ValueError,
        'labels must be at the image resolution (32, 32) or the feature resolution (4, 4), got (5, 5)'),
    ('labels-count', 'stylize_regions'): (ValueError, 'labels has 2 maps for a batch of 1'),
    ('labels-count', 'stylize_regions_wct'): (ValueError, 'labels has 2 maps for a batch of 1'),
    ('labels-count', 'stylize_regions_efdm'): (ValueError, 'labels has 2 maps for a batch of 1'),
    ('labels-count', 'stylize_swap_regions'): (ValueError, 'labels has 2 maps for a batch of 1'),
    ('labels-type', 'stylize_regions'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-type', 'stylize_regions_wct'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-type', 'stylize_regions_efdm'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-type', 'stylize_swap_regions'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-rank', 'stylize_regions'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-rank', 'stylize_regions_wct'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-rank', 'stylize_regions_efdm'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-rank', 'stylize_swap_regions'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('style_labels-resolution', 'stylize_regions'): (ValueError,
        'style_labels must be at the image resolution (32, 32) or the feature resolution (4, 4), got (7, 32)'),
    ('style_labels-resolution', 'stylize_regions_wct'): (ValueError,
        'style_labels must be at the image resolution (32, 32) or the feature resolution (4, 4), got (7, 32)'),
    ('style_labels-resolution', 'stylize_regions_efdm'): (ValueError,
        'style_labels must be at the image resolution (32, 32) or the feature resolution (4, 4), got (7, 32)'),
    ('style_labels-resolution', 'stylize_swap_regions'): (ValueError,
        'style_labels must be at the image resolution (32, 32) or the feature resolution (4, 4), got (7, 32)'),
    ('style_labels-count', 'stylize_regions'): (ValueError, 'style_labels has 2 maps for a batch of 1'),
    ('style_labels-count', 'stylize_regions_wct'): (ValueError, 'style_labels has 2 maps for a batch of 1'),
    ('style_labels-count', 'stylize_regions_efdm'): (ValueError, 'style_labels has 2 maps for a batch of 1'),
    ('style_labels-count', 'stylize_swap_regions'): (ValueError, 'style_labels has 2 maps for a batch of 1'),
    ('style_labels-type', 'stylize_regions'): (ValueError, 'style_labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('style_labels-type', 'stylize_regions_wct'): (ValueError, 'style_labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('style_labels-type', 'stylize_regions_efdm'): (ValueError, 'style_labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('style_labels-type', 'stylize_swap_regions'): (ValueError, 'style_labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-before-style_labels', 'stylize_regions'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-before-style_labels', 'stylize_regions_wct'): (ValueError,
        'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-before-style_labels', 'stylize_regions_efdm'): (ValueError,
        'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-before-style_labels', 'stylize_swap_regions'): (ValueError,
        'labels must be a uint8 tensor [N, H, W] or [H, W]'),
}
OTHER_EXPECT = {
    'forward-preserve_color-under-grad': (NotImplementedError,
        'preserve_color is inference-only; run it under torch.no_grad()'),
    'stylize_swap-under-grad': (NotImplementedError, 'stylize_swap is inference-only; run it under torch.no_grad()'),
    'stylize_with_stats-under-grad': (NotImplementedError,
        'stylize_with_stats is inference-only; run it under torch.no_grad()'),
    'auto_labels-under-grad': (NotImplementedError, 'auto_labels is inference-only; run it under torch.no_grad()'),
    'auto_labels-auto': (ValueError, 'auto must be an AutoRegions, got int'),
    'auto_labels-rank': (ValueError, 'auto_labels needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
}
# a model built with transform="efdm": stylize_regions is refused first, grad or not; the other three run
EFDM_MODEL_EXPECT = {
    ('under-grad', 'stylize_regions'): (NotImplementedError,
        "stylize_regions works on per-channel mean and std, which transform='efdm' does not use; build the model with "
        "transform='adain'; stylize_regions_efdm and stylize_regions_wct take the same arguments whatever the transform"),
    ('under-grad', 'stylize_regions_wct'): (NotImplementedError,
        'stylize_regions_wct is inference-only; run it under torch.no_grad()'),
    ('under-grad', 'stylize_regions_efdm'): (NotImplementedError,
        'stylize_regions_efdm is inference-only; run it under torch.no_grad()'),
    ('under-grad', 'stylize_swap_regions'): (NotImplementedError,
        'stylize_swap_regions is inference-only; run it under torch.no_grad()'),
    ('content-rank', 'stylize_regions'): (NotImplementedError,
        "stylize_regions works on per-channel mean and std, which transform='efdm' does not use; build the model with "
        "transform='adain'; stylize_regions_efdm and stylize_regions_wct take the same arguments whatever the transform"),
    ('content-rank', 'stylize_regions_wct'): (ValueError,
        'stylize_regions_wct needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('content-rank', 'stylize_regions_efdm'): (ValueError,
        'stylize_regions_efdm needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('content-rank', 'stylize_swap_regions'): (ValueError,
        'stylize_swap_regions needs content_img [N, 3, H, W] and style_imgs [S, 3, Hs, Ws]'),
    ('labels-type', 'stylize_regions'): (NotImplementedError,
        "stylize_regions works on per-channel mean and std, which transform='efdm' does not use; build the model with "
        "transform='adain'; stylize_regions_efdm and stylize_regions_wct take the same arguments whatever the transform"),
    ('labels-type', 'stylize_regions_wct'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-type', 'stylize_regions_efdm'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
    ('labels-type', 'stylize_swap_regions'): (ValueError, 'labels must be a uint8 tensor [N, H, W] or [H, W]'),
}


@pytest.fixture(scope="module")
def nets():
    made = {}
    for transform in ("adain", "efdm"):
        made[transform] = models.AdaINStyleTransfer(transform=transform, weights=None)   # never run
        made[transform].encoder = _Relu41Stub()
    return made


@pytest.mark.parametrize("rid,method", [(rid, m) for rid, r in MODEL_ROWS.items() for m in r[0]])
def test_invalid_regional_request_raises_its_type_and_message(rid, method, nets, host_only):
    _, grad, call = MODEL_ROWS[rid]
    kind, message = MODEL_EXPECT[rid, method]
    with torch.set_grad_enabled(grad), pytest.raises(kind) as e:
        call(getattr(nets["adain"], method))
    assert type(e.value) is kind and str(e.value) == message


@pytest.mark.parametrize("rid", list(OTHER_ROWS))
def test_invalid_model_request_raises_its_type_and_message(rid, nets, host_only):
    grad, call = OTHER_ROWS[rid]
    kind, message = OTHER_EXPECT[rid]
    with torch.set_grad_enabled(grad), pytest.raises(kind) as e:
        call(nets["adain"])
    assert type(e.value) is kind and str(e.value) == message


@pytest.mark.parametrize("rid", ["under-grad", "content-rank", "labels-type"])
@pytest.mark.parametrize("method", REGIONAL)
def test_regional_request_on_an_efdm_model(method, rid, nets, host_only):
    _, grad, call = MODEL_ROWS[rid]
    kind, message = EFDM_MODEL_EXPECT[rid, method]
    with torch.set_grad_enabled(grad), pytest.raises(kind) as e:
        call(getattr(nets["efdm"], method))
    assert type(e.value) is kind and str(e.value) == message

"""The dispatcher surface (library.py, csrc/torch_ops.cpp): torch.ops.ast_hip.* runs the same HIP
kernels as the direct C-ABI path, traces under torch.compile(fullgraph=True) without a graph break,
and its registered autograd formulas give the gradients of the autograd.Function path."""
import pytest
import torch

from arbitrarystyletransfer_amd import library, models, synth  # noqa: F401  (library registers the ops)

pytestmark = pytest.mark.gpu


def _imgs(d, n=2, hw=64):
    c = torch.from_numpy(synth.image(31, (n, 3, hw, hw))).to(d)
    s = torch.from_numpy(synth.image(32, (n, 3, hw, hw))).to(d)
    return c, s


def test_compile_fullgraph_style_transfer_bit_identical(hip_device):
    """torch.compile(AdaINStyleTransfer(), fullgraph=True): no graph break (fullgraph raises on
    one), and the compiled forward -- torch.ops.ast_hip.conv3x3 / adain_map with the pack op --
    gives the eager C-ABI path's bits."""
    torch._dynamo.reset()
    m = models.AdaINStyleTransfer().to(hip_device).eval()
    c, s = _imgs(hip_device)
    with torch.no_grad():
        ref = m(c, s, 0.8)
        cm = torch.compile(m, fullgraph=True, dynamic=False)
        out = cm(c, s, 0.8)
        out2 = cm(c, s, 0.8)
    torch.cuda.synchronize()
    assert torch.equal(out, ref) and torch.equal(out2, ref)


def test_explain_reports_no_graph_break(hip_device):
    torch._dynamo.reset()
    m = models.AdaINStyleTransfer().to(hip_device).eval()
    c, s = _imgs(hip_device, hw=48)
    with torch.no_grad():
        ex = torch._dynamo.explain(m)(c, s)
    assert ex.graph_break_count == 0 and ex.graph_count == 1
    names = {str(n.target) for g in ex.graphs for n in g.graph.nodes if n.op == "call_function"}
    assert any("ast_hip.conv3x3" in t for t in names) and any("ast_hip.adain_map" in t for t in names)


def test_conv3x3_op_autograd_matches_function_path(hip_device):
    """ast_hip::conv3x3's registered backward (encoder: zero pad + ReLU/pool taps, and the conv_1
    form with the image normalisation; decoder: upsample + reflect, and the form without ReLU) vs
    functional.EncoderConvFn / DecoderConvFn: both enter the same backward bodies
    (functional.encoder_conv_backward / decoder_conv_backward), same kernels, same bits."""
    from arbitrarystyletransfer_amd import functional as Fn
    from arbitrarystyletransfer_amd import ops
    d = hip_device
    x = (torch.from_numpy(synth.image(41, (2, 32, 24, 20))).to(d) * 2 - 0.5)
    w = torch.from_numpy(synth.conv_weight(42, 48, 32, 3)).to(d)
    b = torch.from_numpy(synth.conv_bias(43, 48)).to(d)
    pk = ops.pack_conv3x3(w)
    g = torch.from_numpy(synth.image(44, (2, 48, 12, 10))).to(d) - 0.5
    for use_op in (True, False):
        xs, ws, bs = (t.clone().requires_grad_() for t in (x, w, b))
        if use_op:
            pre, act, pool = torch.ops.ast_hip.conv3x3(xs, ws, pk, bs, 1, 0, None, None, True, True, True, None)
        else:
            pre, act, pool = Fn.EncoderConvFn.apply(xs, ws, bs, pk, True, True, None, None)
        (pool * g).sum().backward()
        res = (pool.detach(), xs.grad, ws.grad, bs.grad)
        if use_op:
            op_res = res
    for a, r in zip(op_res, res):
        assert torch.equal(a, r)
    gd = torch.from_numpy(synth.image(45, (2, 48, 48, 40))).to(d) - 0.5
    for use_op in (True, False):
        xs, ws, bs = (t.clone().requires_grad_() for t in (x, w, b))
        if use_op:
            _, act, _ = torch.ops.ast_hip.conv3x3(xs, ws, pk, bs, 2, 1, None, None, False, True, False, None)
        else:
            act = Fn.DecoderConvFn.apply(xs, ws, bs, pk, 2, True)
        (act * gd).sum().backward()
        res = (act.detach(), xs.grad, ws.grad, bs.grad)
        if use_op:
            op_res = res
    for a, r in zip(op_res, res):
        assert torch.equal(a, r)
    # the decoder form without ReLU: the gradient reaches the weight-gradient kernel unmasked
    gl = torch.from_numpy(synth.image(46, (2, 48, 24, 20))).to(d) - 0.5
    for use_op in (True, False):
        xs, ws, bs = (t.clone().requires_grad_() for t in (x, w, b))
        if use_op:
            out, _, _ = torch.ops.ast_hip.conv3x3(xs, ws, pk, bs, 1, 1, None, None, True, False, False, None)
        else:
            out = Fn.DecoderConvFn.apply(xs, ws, bs, pk, 1, False)
        (out * gl).sum().backward()
        res = (out.detach(), xs.grad, ws.grad, bs.grad)
        if use_op:
            op_res = res
    for a, r in zip(op_res, res):
        assert torch.equal(a, r)
    # the conv_1 form: the image normalisation in the gather, its scale in the input gradient, and the
    # weight gradient on the normalised image
    x1 = torch.from_numpy(synth.image(47, (2, 3, 24, 20))).to(d)
    w1 = torch.from_numpy(synth.conv_weight(48, 16, 3, 3)).to(d)
    b1 = torch.from_numpy(synth.conv_bias(49, 16)).to(d)
    pk1 = ops.pack_conv3x3(w1)
    mean = torch.tensor([0.485, 0.456, 0.406], device=d)
    std = torch.tensor([0.229, 0.224, 0.225], device=d)
    g1 = torch.from_numpy(synth.image(50, (2, 16, 12, 10))).to(d) - 0.5
    for use_op in (True, False):
        xs, ws, bs = (t.clone().requires_grad_() for t in (x1, w1, b1))
        if use_op:
            pre, act, pool = torch.ops.ast_hip.conv3x3(xs, ws, pk1, bs, 1, 0, mean, std, True, True, True, None)
        else:
            pre, act, pool = Fn.EncoderConvFn.apply(xs, ws, bs, pk1, True, True, mean, std)
        (pool * g1).sum().backward()
        res = (pool.detach(), xs.grad, ws.grad, bs.grad)
        if use_op:
            op_res = res
    for a, r in zip(op_res, res):
        assert torch.equal(a, r)


def test_adain_map_op_autograd_matches_function(hip_device):
    from arbitrarystyletransfer_amd import functional as Fn
    d = hip_device
    c = torch.from_numpy(synth.image(51, (2, 16, 12, 10))).to(d) * 3
    s = torch.from_numpy(synth.image(52, (2, 16, 7, 9))).to(d) + 0.5
    g = torch.from_numpy(synth.image(53, (2, 16, 12, 10))).to(d) - 0.5
    out = []
    for use_op in (True, False):
        cs, ss = c.clone().requires_grad_(), s.clone().requires_grad_()
        t = (torch.ops.ast_hip.adain_map(cs, ss, 0.7, True) if use_op else Fn.AdaINFn.apply(cs, ss, 0.7, True))
        (t * g).sum().backward()
        out.append((t.detach(), cs.grad, ss.grad))
    for a, r in zip(*out):
        assert torch.equal(a, r)

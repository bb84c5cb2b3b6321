"""CPU: the dtype guards of token_linear.py's wrappers, driven without a GPU.

``TokenLinear`` under autocast must be ``nn.Linear``. Before the guard, ``TokenLinear.forward`` looked at ``x`` only; inside
``_TokenLinearFn`` autocast was still active, ``F.linear`` returned bf16, autograd handed the backward a bf16 ``dy`` and
``linear_wgrad`` passed its address to ``psf_linear_wgrad_strided_f32`` beside an f32 ``x``: on that code the recorder below
receives ``(torch.float32, torch.bfloat16)`` (or ``dy.matmul(weight)`` raises first when the input needs a gradient and
``backward()`` runs outside the region), and int32 ids reach ``psf_embed_tokens_bwd_f32(const int64_t* idx, ...)`` as they are.
"""
import contextlib
import re

import pytest
import torch
from torch import nn

import ptr_audit
from sparsefactorization_amd import _lib, token_linear
from sparsefactorization_amd.token_linear import MAX_WIDTH, MIN_TOKENS, TokenEmbedding, TokenLinear

T_ROWS, M_IN, N_OUT = (4, 1025), 8, 5  # 4100 rows: just above MIN_TOKENS


@pytest.fixture
def recorder(monkeypatch):
    """``wgrad_supported`` without its ``is_cuda`` term and ``linear_wgrad`` replaced by a function that notes the dtypes it is
    handed and answers with the gradients themselves."""
    seen = []

    def supported(x2d, out_features):
        return x2d.dtype == torch.float32 and x2d.shape[0] >= MIN_TOKENS and x2d.shape[1] <= MAX_WIDTH and out_features <= MAX_WIDTH

    def linear_wgrad(x2d, dy2d, need_bias=True):
        seen.append((x2d.dtype, dy2d.dtype))
        return dy2d.float().t().mm(x2d.float()), (dy2d.float().sum(0) if need_bias else None)

    monkeypatch.setattr(token_linear, "wgrad_supported", supported)
    monkeypatch.setattr(token_linear, "linear_wgrad", linear_wgrad)
    return seen


def _pair(bias=True):
    torch.manual_seed(3)
    ours, stock = TokenLinear(M_IN, N_OUT, bias=bias), nn.Linear(M_IN, N_OUT, bias=bias)
    stock.load_state_dict(ours.state_dict())
    return ours, stock


def _run(layer, x, amp_dtype, inside):
    """(output, dX or None, dW, db or None) of one forward under autocast and one backward inside or outside the region."""
    x = x.detach().clone().requires_grad_(x.requires_grad)
    layer.zero_grad(set_to_none=True)
    with torch.autocast("cpu", dtype=amp_dtype) if amp_dtype is not None else contextlib.nullcontext():
        out = layer(x)
        loss = (out.float() * torch.arange(1, out.numel() + 1, dtype=torch.float32).reshape(out.shape).remainder(7)).sum()
        if inside:
            loss.backward()
    if not inside:
        loss.backward()
    return out.detach(), x.grad, layer.weight.grad, None if layer.bias is None else layer.bias.grad


def test_without_autocast_the_recorder_is_reached(recorder):
    """(the patched route really leads to ``linear_wgrad``: the autocast cases below do not pass by never getting there)"""
    ours, stock = _pair()
    x = torch.randn(*T_ROWS, M_IN)
    got, want = _run(ours, x, None, False), _run(stock, x, None, False)
    assert recorder == [(torch.float32, torch.float32)]
    assert torch.equal(got[0], want[0])
    torch.testing.assert_close(got[2], want[2], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("inside", [False, True], ids=["backward_outside", "backward_inside"])
@pytest.mark.parametrize("needs_grad", [False, True], ids=["leaf_input", "input_needs_grad"])
@pytest.mark.parametrize("amp_dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_token_linear_under_autocast_is_nn_linear(recorder, amp_dtype, needs_grad, inside):
    ours, stock = _pair()
    x = torch.randn(*T_ROWS, M_IN).requires_grad_(needs_grad)
    got = _run(ours, x, amp_dtype, inside)
    assert not recorder, recorder  # the stock path: linear_wgrad is never asked (before the guard: (float32, bfloat16))
    want = _run(stock, x, amp_dtype, inside)
    assert got[0].dtype == want[0].dtype == amp_dtype
    for g, w, what in zip(got, want, ("output", "dX", "dW", "db")):
        assert (g is None) == (w is None), what
        if g is not None:
            assert g.dtype == w.dtype and torch.equal(g, w), what
    assert (got[1] is not None) == needs_grad and got[2].dtype == torch.float32 and got[3].dtype == torch.float32


def test_no_grad_forward_under_autocast_is_nn_linear(recorder):
    ours, stock = _pair()
    x = torch.randn(*T_ROWS, M_IN)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        got, want = ours(x), stock(x)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want) and not recorder


def test_function_called_directly_with_a_foreign_gradient_raises(monkeypatch):
    """``_TokenLinearFn`` reached past ``TokenLinear.forward`` (``stacked_apply`` calls it) under autocast: the real
    ``linear_wgrad`` refuses the bf16 gradient before it touches the library."""
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    ours, _ = _pair()
    x = torch.randn(*T_ROWS, M_IN)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        out = token_linear._TokenLinearFn.apply(x, ours.weight, ours.bias)
        assert out.dtype == torch.bfloat16
        with pytest.raises(TypeError, match=r"dy is torch\.bfloat16$"):  # the gradient's dtype, not the operands' device
            out.float().sum().backward()


@pytest.mark.parametrize("which", ["x", "dy"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64, torch.float32], ids=["bf16", "f16", "f64", "f32_on_the_cpu"])
def test_linear_wgrad_refuses_foreign_operands_before_the_library(monkeypatch, dtype, which):
    """bf16, f16, f64 and CPU operands: TypeError, raised before ``_lib.load()`` (here a stub that fails on use). The message
    names the operand and what is wrong with it: the element type of either operand is looked at before any device, so on
    these CPU tensors a foreign dtype is refused as a dtype (tests/test_gpu_autocast.py does the same with HIP tensors)."""
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    x, dy = torch.zeros(4100, 8), torch.zeros(4100, 5)
    if which == "x":
        x = x.to(dtype)
    else:
        dy = dy.to(dtype)
    reason = rf"; {which} is {re.escape(str(dtype))}$" if dtype != torch.float32 else r"; x is on 'cpu'$"
    with pytest.raises(TypeError, match="float32 tensors on one HIP device" + reason):
        token_linear.linear_wgrad(x, dy)
    with pytest.raises(TypeError, match=r"; x is torch\.\w+$" if which == "x" and dtype != torch.float32 else r"; dy is <class 'NoneType'>$"):
        token_linear.linear_wgrad(x, None)


class _EmbedStub:
    """The two entries ``embedding_wgrad`` calls; the audit reads what reaches them."""

    def __init__(self):
        self.calls = 0

    def psf_embed_tokens_bwd_workspace(self, T, V, E):
        return 256

    def psf_embed_tokens_bwd_f32(self, *args):
        self.calls += 1
        return 0


@pytest.mark.parametrize("dtype", [torch.int32, torch.int16, torch.uint8, torch.int64], ids=str)
def test_embedding_wgrad_hands_the_entry_int64_ids(monkeypatch, dtype):
    stub = _EmbedStub()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    monkeypatch.setattr(_lib, "stream_ptr", lambda dev: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    idx = torch.arange(40, dtype=torch.int64).remainder(6).to(dtype).reshape(4, 10)
    with ptr_audit.audit(monkeypatch, stub, _lib.SIGNATURES) as a:
        dW = token_linear.embedding_wgrad(idx, torch.ones(4, 10, 8), 6, None)
    assert stub.calls == 1 and a.checked == 4 and not a.violations and dW.shape == (6, 8)  # ids, dOut, dTable, workspace


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=str)
def test_embedding_wgrad_beyond_the_kernel_takes_the_stock_operator(monkeypatch, dtype):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
    vocab = token_linear.EMB_MAX_VOCAB + 1
    idx = torch.arange(40, dtype=torch.int64).mul(13).remainder(vocab).to(dtype)
    dout = torch.arange(40 * 4, dtype=torch.float32).reshape(40, 4)
    want = torch.zeros(vocab, 4).index_add_(0, idx.long(), dout)
    want[7] = 0
    assert torch.equal(token_linear.embedding_wgrad(idx, dout, vocab, 7), want)


def test_token_embedding_on_the_cpu_takes_int32_ids():
    """(CPU tensors take the stock path: the values and the table gradient of int32 ids are those of int64 ids)"""
    torch.manual_seed(5)
    emb = TokenEmbedding(9, 4, padding_idx=7)
    idx = torch.randint(0, 9, (3, 11))
    grads = []
    for ids in (idx, idx.to(torch.int32)):
        emb.zero_grad(set_to_none=True)
        out = emb(ids)
        (out * torch.arange(out.numel(), dtype=torch.float32).reshape(out.shape)).sum().backward()
        grads.append((out.detach(), emb.weight.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])

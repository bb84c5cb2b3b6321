"""GPU: operand types at the Python boundary — the library's own modules under ``torch.autocast`` and with int32 token ids.

The wrappers pass ``tensor.data_ptr()`` to entries typed only by their name, so everything here runs inside
``ptr_audit.audit`` (tests/ptr_audit.py) in its refusing form: a tensor of a dtype the entry does not read fails the test at the
call, before the launch. What must hold ("Autocast and index types"):

* under autocast ``TokenLinear`` is ``nn.Linear`` and the FLATTEN head with more than 8 outputs is ``final(flat)`` — dtype, values
  and gradients bit for bit those of the stock modules, backward inside or outside the region; without autocast the kernels
  still run (their calls are counted);
* ``TokenEmbedding`` / ``embed_tokens`` with int32 ids give the values and the table gradient of int64 ids, the gradient being
  the exact known answer of tests/helper_cases.py;
* the fused routes (narrow and wide producer MLPs, the chain, ``embed_tokens``, the head with at most 8 outputs) call no
  autocast-eligible op and return the float32 bits they return without autocast;
* the models: with int32 ids every parameter gradient at the f32 twin bar (4 x E32); under bf16 autocast every parameter
  gradient float32, finite, with the twin's pattern of absent gradients and exact zeros, on the routes of ``AUTOCAST_ROUTES``,
  within 4 x E_ac — E_ac being the worst per-parameter error of ``psf_twin.forward`` itself (stock PyTorch ops, nothing of this
  package) run on the GPU under the same autocast, against the float64 twin. bf16 carries 8 bits: that bar is a wiring bound
  (a lost or garbage gradient has error >= 1), not a parity bar. Condition on every case: 0 < E_ac <= 0.125; a batch that breaks
  it is passed over for the next batch number (the rule of ``psf_twin.batches_of``), and the number taken is printed. A case
  with no bf16 op on its path (``f32_throughout``) is held to the f32 bar, 4 x E32, as well;
* one f32 training step of every twin case, one eval forward per ``fused_mixer.route`` and the bf16 PSFNet's training step on
  the default and on the opt-in bf16 routes show the audit nothing.

Measured values: profiles/autocast_twin.md.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch
from torch import nn

import helper_cases as H
import psf_twin as T
import ptr_audit
from conftest import rel_inf
from test_gpu_model_twin import Spy, _build, _set_masks, _twin

pytestmark = pytest.mark.gpu

E_AC_MAX = 0.125  # so that no bar exceeds 0.5: a gradient that is all zeros has error 1
AMP = {"bf16": torch.bfloat16, "f16": torch.float16}


@contextlib.contextmanager
def audited(monkeypatch):
    with ptr_audit.audit(monkeypatch, refuse=True) as a:
        yield a
    assert a.checked > 0 and not a.violations  # (the block did reach the library, and through recorded tensors)


def _amp(dtype):
    return torch.autocast("cuda", dtype=dtype) if dtype is not None else contextlib.nullcontext()


def _weights(n):
    """Fixed pseudo-random multipliers in [0, 7) that make every output element's gradient its own."""
    return (torch.arange(n, dtype=torch.float32) * 0.37).remainder(7.0)


# --------------------------------------------------------------------------------------------------------- TokenLinear
def _linear_run(layer, x, needs_grad, amp_dtype, inside):
    x = x.detach().clone().requires_grad_(needs_grad)
    layer.zero_grad(set_to_none=True)
    with _amp(amp_dtype):
        out = layer(x)
        loss = (out.float() * _weights(out.numel()).to(out.device).reshape(out.shape)).sum()
        if inside:
            loss.backward()
    if not inside:
        loss.backward()
    return {"out": out.detach(), "dX": x.grad, "dW": layer.weight.grad, "db": layer.bias.grad}


@pytest.mark.parametrize("amp", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [(4100, 32, 16), (4100, 8, 128), (4100, 2, 30)], ids=lambda s: "x".join(map(str, s)))
def test_token_linear_under_autocast_is_nn_linear(gpu, monkeypatch, shape, amp):
    """T x m x n just above MIN_TOKENS; 4100 x 2 x 30 is K = 2 with a width psf_affine_rows_f32 refuses (30 % 4)."""
    from sparsefactorization_amd.token_linear import TokenLinear
    Tn, m, n = shape
    torch.manual_seed(11)
    ours, stock = TokenLinear(m, n).to(gpu), nn.Linear(m, n).to(gpu)
    stock.load_state_dict(ours.state_dict())
    x = torch.randn(4, Tn // 4, m, device=gpu)
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        for needs_grad in (False, True):
            for inside in (False, True):
                spy.reset()
                got = _linear_run(ours, x, needs_grad, AMP[amp], inside)
                assert not spy.calls, dict(spy.calls)  # the stock path: nothing of the library runs
                want = _linear_run(stock, x, needs_grad, AMP[amp], inside)
                assert got["out"].dtype == AMP[amp] and (got["dX"] is not None) == needs_grad
                for k in got:
                    assert (got[k] is None) == (want[k] is None), k
                    if got[k] is not None:
                        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (k, needs_grad, inside)
        # the same data without autocast: the kernel is still the one that runs, once, and is right
        spy.reset()
        got = _linear_run(ours, x, True, None, False)
        assert spy.calls["psf_linear_wgrad_strided_f32"] == 1, dict(spy.calls)
    x64, dy64 = x.double().reshape(-1, m), _weights(Tn * n).to(gpu).double().reshape(-1, n)
    assert got["out"].dtype == torch.float32
    assert rel_inf(got["dX"].reshape(-1, m).cpu().numpy(), (dy64 @ ours.weight.detach().double()).cpu().numpy()) <= 1e-5
    assert rel_inf(got["dW"].cpu().numpy(), (dy64.t() @ x64).cpu().numpy()) <= 1e-5
    assert rel_inf(got["db"].cpu().numpy(), dy64.sum(0).cpu().numpy()) <= 1e-5


@pytest.mark.parametrize("which", ["x", "dy"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float64], ids=["bf16", "f16", "f64"])
def test_linear_wgrad_refuses_hip_tensors_of_a_foreign_dtype(gpu, monkeypatch, dtype, which):
    """HIP operands, so nothing but the element type is wrong: f32 ``x`` beside a bf16 / f16 / f64 ``dy`` and the reverse. A
    TypeError that names the operand and its dtype, raised before the library is loaded or any entry called (``_lib.load`` fails
    on use; the refusing audit would stop a call that got that far before its launch)."""
    from sparsefactorization_amd import _lib, token_linear
    x, dy = torch.zeros(4100, 8, device=gpu), torch.zeros(4100, 5, device=gpu)
    if which == "x":
        x = x.to(dtype)
    else:
        dy = dy.to(dtype)
    with ptr_audit.audit(monkeypatch, refuse=True) as a:
        monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was touched"))
        with pytest.raises(TypeError, match=rf"float32 tensors on one HIP device; {which} is {str(dtype).replace('.', '[.]')}$"):
            token_linear.linear_wgrad(x, dy)
        # ... and float32 with one operand left on the CPU: refused for the device, and said so
        x32, dy32 = (x.float().cpu(), dy.float()) if which == "x" else (x.float(), dy.float().cpu())
        with pytest.raises(TypeError, match=rf"float32 tensors on one HIP device; {which} is on 'cpu'$"):
            token_linear.linear_wgrad(x32, dy32)
    assert a.checked == 0 and not a.violations


# ----------------------------------------------------------------------------------------------------------- flat head
def _head_run(apply, final, flat, amp_dtype):
    flat = flat.detach().clone().requires_grad_(True)
    final.zero_grad(set_to_none=True)
    with _amp(amp_dtype):
        out = apply(final, flat)
        loss = (out.float() * _weights(out.numel()).to(out.device).reshape(out.shape)).sum()
    loss.backward()  # outside the region
    return {"out": out.detach(), "dX": flat.grad, "dW": final.weight.grad, "db": final.bias.grad}


@pytest.mark.parametrize("amp", ["bf16", "f16"])
@pytest.mark.parametrize("J", [16, 4])
def test_flat_head_under_autocast(gpu, monkeypatch, J, amp):
    """B = 4, K = 4096. J = 16 (GEMM forward inside the Function): under autocast it is ``final(flat)`` bit for bit and its
    backward runs outside the region; J = 4 (the head kernel): float32 logits and gradients, the bits it gives without autocast."""
    from sparsefactorization_amd.psfnet import _flat_head
    torch.manual_seed(12)
    final = nn.Linear(4096, J).to(gpu)
    flat = torch.randn(4, 4096, device=gpu)
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        plain = _head_run(_flat_head, final, flat, None)
        assert spy.calls["psf_flat_head_bwd_f32"] == 1 and spy.calls["psf_flat_head_f32"] == (1 if J <= 8 else 0), dict(spy.calls)
        assert plain["out"].dtype == torch.float32
        spy.reset()
        got = _head_run(_flat_head, final, flat, AMP[amp])
        if J > 8:
            assert not spy.calls, dict(spy.calls)
            want = _head_run(lambda f, x: f(x), final, flat, AMP[amp])
            assert got["out"].dtype == AMP[amp]
        else:
            assert spy.calls["psf_flat_head_f32"] == 1 and spy.calls["psf_flat_head_bwd_f32"] == 1, dict(spy.calls)
            want = plain
            assert got["out"].dtype == torch.float32
    for k in got:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert all(got[k].dtype == torch.float32 for k in ("dX", "dW", "db"))


# ---------------------------------------------------------------------------------------------------------- embeddings
@pytest.mark.parametrize("vocab,pad", [(6, None), (97, 95)])
def test_token_embedding_takes_int32_ids(gpu, monkeypatch, vocab, pad):
    """E = 8, T = 4100 ids as [4, 1025]: the forward of nn.Embedding, and the table gradient for an integer-valued ``dout``
    (helper_cases.EmbGrad: every sum exact in f32 in any order) — the exact answer, the same bits for both id dtypes, the
    padding row exactly zero although its id occurs."""
    from sparsefactorization_amd.token_linear import TokenEmbedding
    case = H.EmbGrad(4100, vocab, 8, "uniform")
    assert case.bound() < H.LIMIT
    ids, dout = torch.from_numpy(case.idx()).reshape(4, 1025).to(gpu), torch.from_numpy(case.dout()).reshape(4, 1025, 8).to(gpu)
    want = case.expected()
    if pad is not None:
        assert (case.idx() == pad).any()
        want[pad] = 0
    want = H.as_f32(want)
    torch.manual_seed(13)
    emb = TokenEmbedding(vocab, 8, padding_idx=pad).to(gpu)
    stock = nn.Embedding(vocab, 8, padding_idx=pad).to(gpu)
    stock.load_state_dict(emb.state_dict())
    spy = Spy(monkeypatch)
    grads = {}
    with audited(monkeypatch):
        for dtype in (torch.int32, torch.int64):
            emb.zero_grad(set_to_none=True)
            spy.reset()
            out = emb(ids.to(dtype))
            assert torch.equal(out, stock(ids))
            out.backward(dout)
            assert spy.calls["psf_embed_tokens_bwd_f32"] == 1, dict(spy.calls)
            grads[dtype] = emb.weight.grad.cpu().numpy()
    assert np.array_equal(grads[torch.int32], grads[torch.int64])
    assert np.array_equal(grads[torch.int32], want)
    if pad is not None:
        assert not grads[torch.int32][pad].any()


def test_embed_tokens_takes_int32_ids(gpu, monkeypatch):
    from sparsefactorization_amd.token_linear import TokenEmbedding, embed_tokens
    torch.manual_seed(14)
    emb = TokenEmbedding(97, 8, padding_idx=95).to(gpu)
    pos = torch.randn(1025, 8, device=gpu, requires_grad=True)
    ids = torch.randint(0, 97, (4, 1025), device=gpu)
    dout = torch.from_numpy(H.EmbGrad(4100, 97, 8, "uniform").dout()).reshape(4, 1025, 8).to(gpu)
    spy = Spy(monkeypatch)
    res = {}
    with audited(monkeypatch):
        for dtype in (torch.int64, torch.int32):
            emb.zero_grad(set_to_none=True)
            pos.grad = None
            spy.reset()
            out = embed_tokens(ids.to(dtype), emb, pos)
            assert spy.calls["psf_embed_tokens_f32"] == (1 if dtype == torch.int64 else 0)
            out.backward(dout)
            assert spy.calls["psf_embed_tokens_bwd_f32"] == 1
            res[dtype] = (out.detach(), emb.weight.grad.clone(), pos.grad.clone())
    assert torch.equal(res[torch.int32][0], res[torch.int64][0])
    assert torch.equal(res[torch.int32][0], emb.weight.detach()[ids] + pos.detach().unsqueeze(0))
    assert torch.equal(res[torch.int32][1], res[torch.int64][1])  # integer-valued dout: exact in any order
    assert torch.equal(res[torch.int32][2], res[torch.int64][2]) and not res[torch.int32][1][95].any()


# ------------------------------------------------------------------------------------------------ the models' plumbing
def _run_model(case, net, gpu, which, ids_dtype=None, amp_dtype=None, inside=False):
    """One forward and backward of the library's network on batch ``which``: {"loss", "grads"} as psf_twin.run_twin returns."""
    net.train()
    x, y, masks = T.make_batch(case, which)
    if ids_dtype is not None:
        assert not x.is_floating_point()
        x = x.to(ids_dtype)
    _set_masks(net, case, masks, gpu)
    with _amp(amp_dtype):
        value = T.loss_of(case.loss, net(x.to(gpu)), y.to(gpu))
        if inside:
            value.backward()
    if not inside:
        value.backward()
    torch.cuda.synchronize()
    return {"loss": float(value.detach()),
            "grads": {n: (None if p.grad is None else p.grad.detach().cpu().numpy()) for n, p in net.named_parameters()},
            "dtypes": {n: p.grad.dtype for n, p in net.named_parameters() if p.grad is not None}}


def test_fused_routes_return_their_float32_bits_under_autocast(gpu, monkeypatch):
    """``embed_tokens``, the narrow and the wide producer MLPs, the chain and the head kernel (J <= 8) call no autocast-eligible op:
    under autocast they take the same routes and return the same float32 bits; bf16 ``data`` with f32 blocks takes no route."""
    from sparsefactorization_amd import fused_mlp
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        for name, amp_dtype in (("order_cls_len", torch.bfloat16), ("order_cls_len", torch.float16), ("listops_like", torch.bfloat16)):
            case = T.CASE[name]
            net = _build(case, gpu).train()
            x, _, masks = T.make_batch(case, 0)
            _set_masks(net, case, masks, gpu)
            fn = net.features if name == "listops_like" else net  # (listops' CLS head is a stock nn.Sequential)
            outs, routes = [], []
            for dt in (None, amp_dtype):
                spy.reset()
                with _amp(dt):
                    outs.append(fn(x.to(gpu)).detach())
                routes.append((list(spy.routes), {k: v for k, v in spy.calls.items() if v}))
            assert outs[1].dtype == torch.float32 and torch.equal(outs[0], outs[1]), name
            assert routes[0] == routes[1] and routes[0][0] == case.routes["mlp"], (name, routes)
        net = _build(T.CASE["order_cls_len"], gpu)
        data = torch.randn(4, 1025, 32, device=gpu)
        with _amp(torch.bfloat16):
            assert fused_mlp.route(data, [net.g, *net.fs]) == "narrow_train"
            assert fused_mlp.route(data.bfloat16(), [net.g, *net.fs]) is None
            assert fused_mlp.apply(data.bfloat16(), [net.g, *net.fs]) is None
            assert net.g(data.bfloat16()).dtype == torch.bfloat16  # the blocks' own layers: nn.Linear under autocast


# ------------------------------------------------------------------------------------------------- models, int32 ids
@pytest.mark.parametrize("name", ["order_cls_len", "imdb_like", "attention_block"])
def test_int32_ids_every_parameter_gradient_matches_the_float64_twin(gpu, monkeypatch, name):
    """``x.to(torch.int32)`` into the library's network; everything stays f32, so the bar is the f32 twin's: 4 x E32, with the
    comparator's checks of the parameters without a gradient and of the exact zeros (the absent id, the padding row)."""
    case = T.CASE[name]
    r64, e32, _ = _twin(name)
    net = _build(case, gpu)
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        got = _run_model(case, net, gpu, T.batches_of(name)[0], ids_dtype=torch.int32)
    verdict = T.compare(got, r64, e32)
    print(f"INT32 {name}: E32 {e32:.3e} bar {verdict.bar:.3e} worst {verdict.worst:.3e} ({verdict.worst / verdict.bar:.2f} x bar) at "
          f"{verdict.worst_name}; calls {dict(spy.calls)}")
    assert spy.calls["psf_embed_tokens_bwd_f32"] == 1 and spy.calls["psf_embed_tokens_f32"] == 0  # ids that are not int64: the stock lookup
    assert len(verdict.errors) == sum(g is not None for g in r64["grads"].values())
    assert not verdict.failures, "\n".join(verdict.failures)


# ------------------------------------------------------------------------------------------------ models under autocast
#: what one training forward + backward under bf16 autocast runs, as observed on an MI355X (profiles/autocast_twin.md); the same
#: for backward() inside and outside the region. ``mlp``: the answers of ``fused_mlp.route``; ``calls``: entry point -> calls.
AUTOCAST_ROUTES = {
    # J = 16 head: the stock nn.Linear (no psf_flat_head_bwd_f32, which the f32 route calls); everything before it f32
    "cifar_like": dict(mlp=["narrow_train"],
                       calls={"psf_embed_tokens_f32": 1, "psf_embed_tokens_bwd_f32": 1, "psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 1,
                              "psf_chord_chain_fwd_f32": 1, "psf_chord_chain_bwd_f32": 1, "psf_flat_head_f32": 0,
                              "psf_flat_head_bwd_f32": 0, "psf_linear_wgrad_strided_f32": 0}),
    # init_linear and the three-layer blocks are nn.Linear: bf16 ``data``, W_m and V0, so the chain is the bf16 chain
    "deep_mlp": dict(mlp=[None, None],
                     calls={"psf_affine_rows_f32": 0, "psf_linear_wgrad_strided_f32": 0, "psf_mlp_fwd_f32": 0, "psf_mlp_fwd_bf16": 0,
                            "psf_chord_chain_fwd_f32": 0, "psf_chord_chain_bwd_f32": 0, "psf_chord_chain_fwd_bf16": 1,
                            "psf_chord_chain_bwd_bf16": 1, "psf_chord_spmm_bwd_bf16": 0, "psf_flat_head_f32": 0,
                            "psf_flat_head_bwd_f32": 0}),
    # every op on its path is a fused f32 route (embed + pos, narrow_train, the chain, the J = 4 head kernel; cross_entropy is
    # on autocast's float32 list): the gradients are the f32 ones and are ALSO held to the f32 twin's bar, 4 x E32
    "order_cls_len": dict(mlp=["narrow_train"], f32_throughout=True,
                          calls={"psf_embed_tokens_f32": 1, "psf_embed_tokens_bwd_f32": 1, "psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 1,
                                 "psf_chord_chain_fwd_f32": 1, "psf_chord_chain_bwd_f32": 1, "psf_flat_head_f32": 1,
                                 "psf_flat_head_bwd_f32": 1}),
    "listops_like": dict(mlp=["wide"],
                         calls={"psf_embed_tokens_f32": 1, "psf_embed_tokens_bwd_f32": 1, "psf_mlp_wide_fwd_f32": 1,
                                "psf_mlp_wide_bwd_f32": 1, "psf_chord_chain_fwd_f32": 1, "psf_chord_chain_bwd_f32": 1,
                                "psf_flat_head_f32": 0, "psf_mlp_fwd_f32": 0}),
    "imdb_like": dict(mlp=["narrow_train"],
                      calls={"psf_embed_tokens_f32": 1, "psf_embed_tokens_bwd_f32": 1, "psf_mlp_fwd_f32": 1, "psf_mlp_bwd_f32": 1,
                             "psf_chord_chain_fwd_f32": 1, "psf_chord_chain_bwd_f32": 1, "psf_flat_head_f32": 0}),
}


def _twin_under_autocast(case, gpu, which, inside):
    """Gradients of ``psf_twin.forward`` — stock PyTorch ops, nothing of this package — with f32 parameters on the GPU under
    bf16 autocast, on batch ``which``."""
    sd = {k: v.to(gpu).clone().requires_grad_(True) for k, v in T.init_state(case).items()}
    x, y, masks = T.make_batch(case, which)
    masks = {k: m.to(gpu) for k, m in masks.items()}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        value = T.loss_of(case.loss, T.forward(case.kind, case.cfg, sd, x.to(gpu), masks, True), y.to(gpu))
        if inside:
            value.backward()
    if not inside:
        value.backward()
    return {"loss": float(value.detach()), "grads": {k: (None if v.grad is None else v.grad.cpu().numpy()) for k, v in sd.items()}}


@functools.lru_cache(maxsize=None)
def _autocast_reference(name, inside):
    """(batch number, float64 twin's run, E_ac, the parameter that sets it): the first batch number from the case's own on whose
    E_ac passes 0 < E_ac <= E_AC_MAX. Nothing of the library enters."""
    case, gpu = T.CASE[name], torch.device("cuda:0")
    first = T.batches_of(name)[0]
    for which in range(first, first + 8):
        r64 = _twin(name)[0] if which == first else T.run_twin(case, torch.float64, batches=(which,))
        errs = T.per_param_error(_twin_under_autocast(case, gpu, which, inside)["grads"], r64["grads"])
        worst = max(errs, key=errs.get)
        print(f"AUTOCAST-REF {name} backward_{'inside' if inside else 'outside'} batch {which}: E_ac {errs[worst]:.3e} at {worst}")
        if 0 < errs[worst] <= E_AC_MAX:
            return which, r64, errs[worst], worst
    raise AssertionError(f"{name}: no batch in {first}..{first + 7} with 0 < E_ac <= {E_AC_MAX}")


@pytest.mark.parametrize("inside", [False, True], ids=["backward_outside", "backward_inside"])
@pytest.mark.parametrize("name", list(AUTOCAST_ROUTES))
def test_models_under_bf16_autocast(gpu, monkeypatch, name, inside):
    case = T.CASE[name]
    which, r64, e_ac, set_by = _autocast_reference(name, inside)
    assert 0 < e_ac <= E_AC_MAX
    net = _build(case, gpu)
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        got = _run_model(case, net, gpu, which, amp_dtype=torch.bfloat16, inside=inside)  # (no exception)
    verdict = T.compare(got, r64, e_ac)
    print(f"AUTOCAST {name} backward_{'inside' if inside else 'outside'}: batch {which} E_ac {e_ac:.3e} (set by {set_by}) bar {verdict.bar:.3e} "
          f"worst {verdict.worst:.3e} ({verdict.worst / verdict.bar:.2f} x bar) at {verdict.worst_name}")
    print(f"AUTOCAST-ROUTES {name} backward_{'inside' if inside else 'outside'}: mlp {spy.routes} calls {dict(spy.calls)}")
    assert all(dt == torch.float32 for dt in got["dtypes"].values()), got["dtypes"]
    assert all(np.isfinite(g).all() for g in got["grads"].values() if g is not None)
    assert len(verdict.errors) == sum(g is not None for g in r64["grads"].values())  # nothing skipped
    assert not verdict.failures, "\n".join(verdict.failures)  # absent gradients, exact zeros, every parameter within 4 x E_ac
    want = AUTOCAST_ROUTES[name]
    if want.get("f32_throughout"):
        r64_f, e32, _ = _twin(name) if which == T.batches_of(name)[0] else _twin(name, None, (which,), None)
        sharp = T.compare(got, r64_f, e32)
        print(f"AUTOCAST-F32 {name}: E32 {e32:.3e} bar {sharp.bar:.3e} worst {sharp.worst:.3e} ({sharp.worst / sharp.bar:.2f} x bar) at {sharp.worst_name}")
        assert not sharp.failures, "\n".join(sharp.failures)
    assert spy.routes == want["mlp"], spy.routes
    for entry, n in want["calls"].items():
        assert spy.calls[entry] == n, (entry, spy.calls[entry], n)


# ---------------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_audit_sweep_f32_training_step_and_eval_routes(gpu, monkeypatch, name):
    """One f32 training step (forward, backward, ``make_adam`` step) of every twin case and one eval forward per
    ``fused_mixer.route``: every tensor whose address reaches the library has the dtype its entry reads."""
    from sparsefactorization_amd import fused_mixer
    from sparsefactorization_amd.train import make_adam
    case = T.CASE[name]
    net = _build(case, gpu)
    opt = make_adam(net.parameters(), 1e-3)
    with audited(monkeypatch) as a:
        _run_model(case, net, gpu, 0)
        opt.step()
        trained = a.checked
        net.eval()
        x, _, _ = T.make_batch(case, 0)
        for route in ("auto", "never", "always"):
            monkeypatch.setattr(fused_mixer, "route", route)
            with torch.no_grad():
                net(x.to(gpu))
        torch.cuda.synchronize()
    assert trained > 0 and a.checked > trained


@pytest.mark.parametrize("routes", ["never", "always"])
def test_audit_sweep_bf16_psfnet_training_step(gpu, monkeypatch, routes):
    """The bf16 PSFNet of test_psfnet_in_bf16 (tests/test_gpu_bf16.py), one training step and one no-grad forward, with the three
    opt-in bf16 routes (producer backward, one-launch backward chain, one-launch mixer) off and on."""
    from sparsefactorization_amd import chord, fused_mixer, fused_mlp
    from sparsefactorization_amd.synthetic_psf import PSFNet
    torch.manual_seed(42)
    cfg = dict(vocab_size=1, add_init_linear_layer=True, embedding_size=32, n_vec=128, n_W=7, Ws=[32, 'GELU'],
               V=[32, 'GELU'], n_channels_V=8, n_class=1, pooling_type="FLATTEN", head=['linear'],
               use_cuda=True, use_residuals=True, use_pos_embedding=False, problem="adding")
    net = PSFNet(**cfg).to(gpu).to(torch.bfloat16)
    x = torch.rand(8, 128, 2, device=gpu).to(torch.bfloat16)
    monkeypatch.setattr(fused_mlp, "bf16_train_route", routes)
    monkeypatch.setattr(chord, "bf16_chain_bwd_route", routes)
    monkeypatch.setattr(fused_mixer, "bf16_route", routes)
    spy = Spy(monkeypatch)
    with audited(monkeypatch):
        out = net(x)
        out.float().sum().backward()
        with torch.no_grad():
            net(x)
        torch.cuda.synchronize()
    print(f"SWEEP-BF16 routes={routes}: mlp {spy.routes} calls {dict(spy.calls)}")
    on = routes == "always"
    assert spy.calls["psf_mlp_bwd_bf16"] == (1 if on else 0) and spy.calls["psf_chord_chain_bwd_lds_bf16"] == (1 if on else 0)
    assert spy.calls["psf_mixer_fwd_bf16"] == (1 if on else 0)
    assert all(p.grad is None or (p.grad.dtype == torch.bfloat16 and torch.isfinite(p.grad).all()) for p in net.parameters())

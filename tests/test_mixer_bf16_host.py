"""CPU: the single-launch bf16 mixer's host side (psf_mixer_fwd_bf16*, include/psf_chord.h; csrc/mixer_lds_bf16_inst.hip:
plan_mixer_lds_bf16) — the limits and one past each of them, the workspace size, every rejection that is documented to come
before the first HIP call, and the Python gate (fused_mixer.bf16_route). Nothing is launched here."""
import ctypes

import pytest
import torch

i32, vp = ctypes.c_int32, ctypes.c_void_p
E_NULL, E_SHAPE, E_ALIAS, E_ALIGN, E_UNSUPPORTED = -1, -2, -3, -4, -7
IMG = 6912  # bytes per unit image (csrc/mlp_bf16_image.h)


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def _h(M, width=32):
    return (i32 * (M + 1))(*([width] * (M + 1)))


def _both(lib, N, E, M, h, C, L):
    """(plan, workspace) of a shape; the two must agree on whether it is covered."""
    plan, ws = lib.psf_mixer_fwd_bf16_plan(N, E, M, h, C, L), lib.psf_mixer_fwd_bf16_workspace(N, E, M, h, C, L)
    assert (plan == 2 and ws > 0) or (plan == 0 and ws == -1), (N, E, M, C, L, plan, ws)
    return plan, ws


# (N, E, M, hidden width, C, L) -> covered? The limits and one past each; the base is Adding's N = 128 network.
LIMITS = [
    ((128, 32, 7, 32, 8, 8), True),
    ((32, 32, 7, 32, 8, 8), True), ((512, 32, 7, 32, 8, 8), True), ((512, 64, 31, 128, 16, 20), True),
    ((544, 32, 7, 32, 8, 8), False), ((1024, 32, 7, 32, 8, 8), False), ((100, 32, 7, 32, 8, 8), False), ((0, 32, 7, 32, 8, 8), False),
    ((128, 32, 7, 32, 16, 8), True), ((128, 32, 7, 32, 4, 8), False), ((128, 32, 7, 32, 32, 8), False), ((128, 32, 7, 32, 12, 8), False),
    ((128, 8, 7, 32, 8, 8), True), ((128, 64, 7, 32, 8, 8), True), ((128, 72, 7, 32, 8, 8), False), ((128, 12, 7, 32, 8, 8), False),
    ((128, 0, 7, 32, 8, 8), False),
    ((128, 32, 7, 128, 8, 8), True), ((128, 32, 7, 129, 8, 8), False), ((128, 32, 7, 1, 8, 8), True), ((128, 32, 7, 0, 8, 8), False),
    ((128, 32, 7, 32, 8, 3), False), ((128, 32, 7, 32, 8, 4), True), ((128, 32, 7, 32, 8, 20), True), ((128, 32, 7, 32, 8, 21), False),
    ((128, 32, 0, 32, 8, 8), False), ((128, 32, 1, 32, 8, 8), True), ((128, 32, 31, 32, 8, 8), True), ((128, 32, 32, 32, 8, 8), False),
]


@pytest.mark.parametrize("shape,covered", LIMITS, ids=["-".join(map(str, s)) for s, _ in LIMITS])
def test_limits_and_one_past_each(lib, shape, covered):
    N, E, M, width, C, L = shape
    plan, ws = _both(lib, N, E, M, _h(max(M, 0), width), C, L)
    assert plan == (2 if covered else 0)
    if covered:
        assert ws == (M + 1) * ((width + 31) // 32) * IMG


def test_h_table_null_and_one_wide_entry(lib):
    assert lib.psf_mixer_fwd_bf16_plan(128, 32, 7, None, 8, 8) == 0
    assert lib.psf_mixer_fwd_bf16_workspace(128, 32, 7, None, 8, 8) == -1
    h = _h(7)
    h[5] = 129  # one MLP past the limit is enough
    assert _both(lib, 128, 32, 7, h, 8, 8) == (0, -1)


def test_workspace_is_one_image_per_32_hidden_rows(lib):
    for widths in ([32] * 8, [7, 32, 33, 128], [128] * 32, [1, 64, 65, 96, 97]):
        h = (i32 * len(widths))(*widths)
        want = sum((w + 31) // 32 for w in widths) * IMG
        assert lib.psf_mixer_fwd_bf16_workspace(128, 32, len(widths) - 1, h, 8, 12) == want
        assert lib.psf_mixer_fwd_bf16_workspace(512, 64, len(widths) - 1, h, 16, 20) == want  # N, E, C, L do not enter


def test_entry_rejects_before_touching_the_gpu(lib):
    """NULL first, then B and the shape, then alignment, then the workspace, then the per-MLP and per-step pointers; the codes
    are the documented ones and the message names the entry. The pointers are fakes: a call that got past validation would
    fault, so every line below also shows that nothing was launched."""
    f = lib.psf_mixer_fwd_bf16
    h = _h(2)
    ws = 3 * IMG
    assert lib.psf_mixer_fwd_bf16_workspace(128, 32, 2, h, 8, 8) == ws
    one, two, three = vp(16), vp(32), vp(48)
    tab = (vp * 3)(16, 16, 16)
    outs = (vp * 2)(64, 80)

    def call(X=one, B=1, N=128, E=32, M=2, A=tab, a=tab, Bw=tab, b=tab, hh=h, C=8, L=8, V0=two, o=outs, w=three, wb=ws):
        return f(X, B, N, E, M, A, a, Bw, b, hh, C, L, 1, V0, o, w, wb, None)

    for kw in (dict(X=None), dict(A=None), dict(a=None), dict(Bw=None), dict(b=None), dict(hh=None), dict(o=None), dict(w=None)):
        assert call(**kw) == E_NULL, kw
        assert b"psf_mixer_fwd_bf16" in lib.psf_last_error()
    assert call(B=-1) == E_SHAPE
    assert call(N=544) == E_UNSUPPORTED and b"psf_chord_chain_fwd_bf16" in lib.psf_last_error()
    assert call(N=1024) == E_UNSUPPORTED
    assert call(C=32) == E_UNSUPPORTED
    assert call(E=12) == E_UNSUPPORTED
    assert call(N=544, X=vp(20)) == E_UNSUPPORTED   # the shape is looked at before the alignment
    assert call(X=vp(20)) == E_ALIGN and b"X" in lib.psf_last_error()
    assert call(X=vp(24)) == E_ALIGN                # 8-byte aligned is not enough
    assert call(V0=vp(40)) == E_ALIGN and b"V0" in lib.psf_last_error()
    assert call(X=vp(20), wb=ws - 16) == E_ALIGN    # ... and the alignment before the workspace
    assert call(wb=ws - 16) == E_SHAPE and b"workspace" in lib.psf_last_error()
    assert call(w=vp(40)) == E_SHAPE                # workspace not 16-byte aligned
    assert call(A=(vp * 3)(16, None, 16)) == E_NULL and b"MLP 1" in lib.psf_last_error()
    assert call(b=(vp * 3)(16, 16, 17)) == E_ALIGN and b"2-byte" in lib.psf_last_error()
    assert call(o=(vp * 2)(64, None)) == E_NULL
    assert call(o=(vp * 2)(64, 72)) == E_ALIGN and b"step 1" in lib.psf_last_error()
    assert call(o=(vp * 2)(32, 80)) == E_ALIAS      # out aliases V0
    assert call(o=(vp * 2)(64, 64)) == E_ALIAS      # a step's input is its output
    assert call(B=0) == 0                           # an empty batch passes validation and launches nothing
    assert call(B=0, V0=None) == 0                  # V0 may be NULL


def test_knob_mixer_lds_takes_the_route_away(lib):
    from sparsefactorization_amd._lib import tuning
    h = _h(2)
    tab, outs = (vp * 3)(16, 16, 16), (vp * 2)(64, 80)
    assert lib.psf_mixer_fwd_bf16_plan(128, 32, 2, h, 8, 8) == 2
    with tuning(mixer_lds=0):
        assert lib.psf_mixer_fwd_bf16_plan(128, 32, 2, h, 8, 8) == 0
        assert lib.psf_mixer_fwd_bf16_workspace(128, 32, 2, h, 8, 8) == 3 * IMG  # the size is the shape's, knob or not
        rc = lib.psf_mixer_fwd_bf16(vp(16), 1, 128, 32, 2, tab, tab, tab, tab, h, 8, 8, 1, vp(32), outs, vp(48), 3 * IMG, None)
        assert rc == E_UNSUPPORTED and b"mixer_lds" in lib.psf_last_error()
    assert lib.psf_mixer_fwd_bf16_plan(128, 32, 2, h, 8, 8) == 2
    assert lib.psf_version() == 2  # additive: no ABI version change


def test_python_gate(lib, monkeypatch):
    """bf16_route is "never" by default; covered_bf16 wants bf16 data on the GPU and bf16 blocks; find_bf16 additionally wants
    the route switched on and nothing needing a gradient. The f32 helper keeps its three-argument form."""
    from sparsefactorization_amd import fused_mixer
    from sparsefactorization_amd.psfnet import MLPBlock
    assert fused_mixer.bf16_route == "never"
    g32, fs32 = MLPBlock([32, 'GELU'], 32, 8), [MLPBlock([32, 'GELU'], 32, 12) for _ in range(3)]
    g16 = MLPBlock([32, 'GELU'], 32, 8).to(torch.bfloat16)
    fs16 = [MLPBlock([32, 'GELU'], 32, 12).to(torch.bfloat16) for _ in range(3)]
    x32, x16 = torch.zeros(2, 64, 32), torch.zeros(2, 64, 32, dtype=torch.bfloat16)
    assert fused_mixer._block_pairs(32, g32, fs32) is not None and fused_mixer._block_pairs(32, g16, fs16) is None
    assert fused_mixer._block_pairs(32, g16, fs16, torch.bfloat16)[0][2:] == (8, 12)
    for x, g, fs in ((x32, g32, fs32), (x16, g32, fs32), (x16, g16, fs16), (x32, g16, fs16)):  # CPU tensors
        assert not fused_mixer.covered_bf16(x, g, fs)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))  # everything but the device
    assert not fused_mixer.covered_bf16(x32, g32, fs32) and not fused_mixer.covered_bf16(x16, g32, fs32)
    assert not fused_mixer.covered_bf16(x32, g16, fs16)
    assert fused_mixer.covered_bf16(x16, g16, fs16)
    assert not fused_mixer.covered_bf16(x16[:, :50], g16, fs16)          # N = 50
    assert not fused_mixer.covered_bf16(x16.reshape(128, 32), g16, fs16)  # not [B, N, E]
    mixed = [fs16[0], fs16[1], MLPBlock([32, 'GELU'], 32, 12).to(torch.bfloat16)]
    mixed[2].network[2].bias.data = mixed[2].network[2].bias.data.float()  # one f32 parameter
    assert not fused_mixer.covered_bf16(x16, g16, mixed)
    with torch.no_grad():
        assert fused_mixer.find_bf16(x16, g16, fs16) is None             # "never"
        monkeypatch.setattr(fused_mixer, "bf16_route", "always")
        found = fused_mixer.find_bf16(x16, g16, fs16)
        assert found is not None and (found[0][0], list(found[0][1]), found[0][2], found[0][3]) == (3, [32] * 4, 8, 12)
        assert fused_mixer.find_bf16(x16, g32, fs32) is None
    assert fused_mixer.find_bf16(x16, g16, fs16) is None                 # the parameters want gradients
    monkeypatch.undo()
    with pytest.raises(ValueError, match="does not cover this call"):
        fused_mixer.mixer_forward_bf16(x16, g16, fs16, True)

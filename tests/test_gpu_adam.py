"""GPU: psf_adam_step_f32 (csrc/adam.hip) called directly.

  a. exact known answers (Adam's first-step rule on operands whose every intermediate is exact): bit for bit, through the
     vector path and through the scalar path
  b. m', v' and p' inside the first-order error envelope of tests/adam_cases.py around the float64 update, at t = 1, 2, 3, 10,
     1000, 100000 (the CPU half, test_adam_cases_cpu.py, shows the envelope holds a float32 emulation with a factor 2 to spare
     and rejects three defects)
  c. lists of 0, 1, 39, 40, 41, 80 and 81 tensors (40 go into one launch) of sizes around the 4096-element chunk, empty ones
     among them, at 0, 4 and 8 bytes off a 16-byte boundary, inside NaN bands: every tensor gets the bits it gets alone
  d. an invalid tensor behind the first launch's 40: the error code, and no tensor has changed
"""
import ctypes

import numpy as np
import pytest
import torch

import adam_cases as ac

pytestmark = pytest.mark.gpu

BAND = 64  # floats: 256 bytes of NaN between and around the tensors
PSF_E_NULL, PSF_E_ALIGN = -1, -4


def _lib():
    from sparsefactorization_amd import _lib
    return _lib.load()


def _call(gpu, tensors, sizes, h, step, step_dev=None, count=None, patch=None):
    """tensors: four lists (p, g, m, v) of device views (or raw addresses). `patch(tables, sizes)` may spoil the tables."""
    vp = ctypes.c_void_p
    n = len(sizes)
    addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()  # noqa: E731
    tabs = [[addr(t) for t in kind] for kind in tensors]
    sizes = list(sizes)
    if patch is not None:
        patch(tabs, sizes)
    ctabs = [(vp * max(n, 1))(*t) for t in tabs]
    return _lib().psf_adam_step_f32(*ctabs, (ctypes.c_int64 * max(n, 1))(*sizes), n if count is None else count, h["lr"], h["beta1"],
                                    h["beta2"], h["eps"], float(step), None if step_dev is None else step_dev.data_ptr(),
                                    torch.cuda.current_stream(gpu).cuda_stream)


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32).numpy().view(np.uint32)


def _shifted(a, gpu, shift):
    """The array as a device view `shift` floats off a 16-byte boundary."""
    buf = torch.zeros(a.size + 8, device=gpu)
    view = buf[shift:shift + a.size]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * shift
    return view


# ---------------------------------------------------------------- a. exact known answers
@pytest.mark.parametrize("path", ["vector", "scalar_pointer", "scalar_size"])
@pytest.mark.parametrize("zero_gradient", [False, True], ids=["first_step_rule", "zero_gradient"])
def test_known_answers_bit_for_bit(gpu, zero_gradient, path):
    """p' = p - 2^-7 sign(g), m' = g / 2, v' = g^2 / 4; with g = 0 and eps = 2^-10 nothing moves and nothing is NaN. The vector path
    needs all four pointers 16-byte aligned and n % 4 == 0: one float off (which torch never hands out), or n = 2047, is scalar."""
    p, g, m, v, h, wp, wm, wv = ac.known_answer(zero_gradient)
    n = p.size if path != "scalar_size" else p.size - 1
    shift = 1 if path == "scalar_pointer" else 0
    dev = [_shifted(a[:n], gpu, shift) for a in (p, g, m, v)]
    assert _call(gpu, [[t] for t in dev], [n], ac.hyper(**h), 1) == 0
    for name, got, want in zip("pmv", (dev[0], dev[2], dev[3]), (wp, wm, wv)):
        bad = int((_bits(got) != want[:n].view(np.uint32)).sum())
        assert bad == 0, f"{name}': {bad} of {n} elements differ"
    assert np.array_equal(_bits(dev[1]), g[:n].view(np.uint32))


# ---------------------------------------------------------------- b. envelope against float64
@pytest.mark.parametrize("t", ac.STEPS)
def test_update_sits_inside_the_first_order_envelope(gpu, t):
    """Measured on the MI355X: the largest error as a share of its bound for p', m', v'; then the largest relative error of v' and,
    on the elements in the first-step state (p = m = v = 0), of the update itself:
        t = 1        0.487  0.210  0.239    1.14e-07  2.28e-07
        t = 2        0.487  0.206  0.240    1.15e-07  3.54e-06
        t = 3        0.488  0.200  0.242    1.15e-07  3.45e-06
        t = 10       0.495  0.206  0.241    1.15e-07  4.05e-07
        t = 1000     0.494  0.210  0.242    1.15e-07  2.25e-07
        t = 100000   0.492  0.209  0.243    1.16e-07  1.83e-07
    The shares equal those of the uncontracted float32 emulation to the digits shown (the library is built without contraction)."""
    h = ac.hyper()
    ops = ac.operands(t)
    want, E = ac.bounds(*ops, h, t)
    dev = [torch.from_numpy(a).to(gpu) for a in ops]
    assert _call(gpu, [[d] for d in dev], [ops[0].size], h, t) == 0
    got = tuple(d.cpu().numpy() for d in (dev[0], dev[2], dev[3]))
    assert all(np.isfinite(a).all() for a in got)
    wp, wm, wv = ac.worst(got, want, E)
    v_rel, upd = ac.measured(got, ops, want)
    print(f"ADAM_ENVELOPE t={t}: of the bound p {wp:.3f} m {wm:.3f} v {wv:.3f}; max rel v' {v_rel:.2e} first-step update {upd:.2e}")
    assert wm <= 1.0, f"m': {wm:.3f} of (2 c1 + 1) U (|m| + |g|)"
    assert wv <= 1.0, f"v': {wv:.3f} of 4 U v'"
    assert wp <= 1.0, f"p': {wp:.3f} of the bound"


# ---------------------------------------------------------------- c. partition and bands
SIZES = (0, 1, 3, 4, 5, 4095, 4096, 4097, 8191, 12288, 12292)
COUNTS = (0, 1, 39, 40, 41, 80, 81)
# floats off a 16-byte boundary for (p, g, m, v): all aligned, all 4 or 8 bytes off, and one array alone off
SHIFTS = ((0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (0, 1, 0, 0), (0, 0, 0, 2), (0, 0, 0, 0))
EMPTY = (0, 20, 38, 39, 40, 80)  # empty tensors: first, in the middle, and last of the lists of 39, 40, 41 and 81


def _sizes():
    s = [SIZES[(7 * k + 3) % len(SIZES)] for k in range(81)]
    for k in EMPTY:
        s[k] = 0
    assert set(s) == set(SIZES)
    return s


class _Arenas:
    """p, g, m, v of 81 tensors, each kind in one NaN-filled buffer with >= BAND floats of NaN around every tensor."""

    def __init__(self, gpu, sizes, seed=3):
        rng = np.random.default_rng(seed)
        self.sizes, self.spans, host = sizes, [[], [], [], []], []
        for kind in range(4):
            cur = 0
            for k, n in enumerate(sizes):
                lo = (cur + BAND + 3) // 4 * 4 + SHIFTS[k % len(SHIFTS)][kind]
                self.spans[kind].append((lo, lo + n))
                cur = lo + n
            a = np.full(cur + BAND, np.nan, dtype=np.float32)
            for lo, hi in self.spans[kind]:
                x = rng.standard_normal(hi - lo)
                a[lo:hi] = {0: x, 1: x * 10.0 ** rng.uniform(-3, 1, hi - lo), 2: 0.1 * x, 3: x * x + 1e-6}[kind]
            host.append(a)
        self.host = host
        self.buf = [torch.from_numpy(a).to(gpu) for a in host]
        assert all(b.data_ptr() % 16 == 0 for b in self.buf)

    def views(self, buf=None):
        """Addresses, not torch views: an empty view has no data_ptr, and an empty tensor of a list still has an address."""
        buf = self.buf if buf is None else buf
        return [[b.data_ptr() + 4 * lo for lo, _hi in spans] for b, spans in zip(buf, self.spans)]

    def vector_path(self, k):
        return all(self.spans[kind][k][0] % 4 == 0 for kind in range(4)) and self.sizes[k] % 4 == 0


@pytest.fixture(scope="module")
def partition(gpu):
    """(arenas as built, their bits after every tensor was updated ALONE by a count = 1 call at the same alignment)."""
    ar = _Arenas(gpu, _sizes())
    alone = [b.clone() for b in ar.buf]
    v = ar.views(alone)
    h = ac.hyper()
    for k, n in enumerate(ar.sizes):
        assert _call(gpu, [[v[kind][k]] for kind in range(4)], [n], h, 3) == 0
    return ar, [_bits(b) for b in alone]


def test_partition_lists_reach_both_paths_in_one_launch(partition):
    ar, _alone = partition
    for base in (0, 40):
        paths = {ar.vector_path(k) for k in range(base, base + 40) if ar.sizes[k]}
        assert paths == {True, False}
    assert any(ar.vector_path(k) and ar.sizes[k] > 4096 for k in range(81))
    assert any(not ar.vector_path(k) and ar.sizes[k] % 4 == 0 and ar.sizes[k] > 4096 for k in range(81))  # scalar by its pointer alone


@pytest.mark.parametrize("count", COUNTS)
def test_every_tensor_of_a_list_gets_the_bits_it_gets_alone(gpu, partition, count):
    ar, alone = partition
    buf = [torch.from_numpy(a).to(gpu) for a in ar.host]
    views = ar.views(buf)
    assert _call(gpu, [kind[:count] for kind in views], ar.sizes[:count], ac.hyper(), 3) == 0
    for kind, name in enumerate("pgmv"):
        got, first = _bits(buf[kind]), ar.host[kind].view(np.uint32)
        inside = np.zeros(got.size, dtype=bool)
        for k, (lo, hi) in enumerate(ar.spans[kind]):
            inside[lo:hi] = True
            want = alone[kind][lo:hi] if k < count and name != "g" else first[lo:hi]
            assert np.array_equal(got[lo:hi], want), f"{name} of tensor {k} (n = {hi - lo}, vector path {ar.vector_path(k)})"
            assert name == "g" or k >= count or hi == lo or not np.array_equal(got[lo:hi], first[lo:hi]), f"{name} of tensor {k} was not updated"
        f = got.view(np.float32)
        assert np.isnan(f[~inside]).all(), f"{name}: a band was written to"
        assert not np.isnan(f[inside]).any(), f"{name}: NaN inside a tensor"


def test_device_step_count_gives_the_bits_of_the_host_one_and_wins(gpu, partition):
    ar, alone = partition
    buf = [torch.from_numpy(a).to(gpu) for a in ar.host]
    step_dev = torch.tensor([3.0], device=gpu)
    assert _call(gpu, ar.views(buf), ar.sizes, ac.hyper(), 7, step_dev=step_dev) == 0
    for kind in (0, 2, 3):
        assert np.array_equal(_bits(buf[kind]), alone[kind])
    other = [torch.from_numpy(a).to(gpu) for a in ar.host]
    assert _call(gpu, ar.views(other), ar.sizes, ac.hyper(), 7) == 0
    assert not np.array_equal(_bits(other[0]), alone[0])  # (t = 7 is another update than t = 3)


# ---------------------------------------------------------------- d. an invalid tensor behind the first launch
@pytest.mark.parametrize("at", [40, 79, 80])
@pytest.mark.parametrize("fault", ["null", "negative_size", "misaligned"])
def test_an_invalid_tensor_anywhere_in_the_list_leaves_every_tensor_unchanged(gpu, partition, fault, at):
    """The whole list is validated before the first launch, so a failed optimizer step is not half applied."""
    ar, _alone = partition
    buf = [torch.from_numpy(a).to(gpu) for a in ar.host]

    def patch(tabs, sizes):
        if fault == "null":
            tabs[2][at] = None
        elif fault == "negative_size":
            sizes[at] = -1
        else:
            tabs[3][at] += 2

    rc = _call(gpu, ar.views(buf), ar.sizes, ac.hyper(), 3, patch=patch)
    torch.cuda.synchronize()
    assert rc == (PSF_E_ALIGN if fault == "misaligned" else PSF_E_NULL)
    for kind, name in enumerate("pgmv"):
        changed = int((_bits(buf[kind]) != ar.host[kind].view(np.uint32)).sum())
        assert changed == 0, f"{name}: {changed} elements changed by a call that returned {rc}"

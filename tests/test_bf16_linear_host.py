"""CPU: ``token_linear.bf16_linear_route`` and the two entries behind it, as far as the host goes.

  the switch         "never" by default; anything but "never" / "always" raises ValueError where it is consulted
  --bf16-linear      needs --bf16; ``--problem adding --bf16`` alone keeps exiting with its message
  stock module       CPU operands and autocast take nn.Linear itself at "always": same bits, no library call
  TypeErrors         linear_wgrad names the operand that is of a mixed or foreign dtype, at "never" and at "always"
  header             include/psf_chord.h with the new declarations is strict C99; a C program links the library, reads the
                     workspace size and gets the argument-error codes of both entries, all before any HIP call
"""
import os
import shutil
import subprocess

import pytest
import torch
from torch import nn

from conftest import ROOT

import linear_wgrad_bf16_cases as C

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from sparsefactorization_amd import _lib, build
    build.build()
    return _lib.load()


def test_switch_defaults_to_never_and_is_validated(monkeypatch):
    from sparsefactorization_amd import token_linear as tl
    assert tl.bf16_linear_route == "never"
    x = torch.zeros(8192, 32, dtype=BF16)
    assert tl.wgrad_supported(x, 32) is False
    monkeypatch.setattr(tl, "bf16_linear_route", "auto")
    w = torch.zeros(8, 2, dtype=BF16)
    with pytest.raises(ValueError, match="bf16_linear_route"):
        tl.affine_rows_supported(torch.zeros(4, 2, dtype=BF16), w, None)
    with pytest.raises(ValueError, match="bf16_linear_route"):
        tl.linear_wgrad(x, x)
    # f32 operands never consult it
    assert tl.affine_rows_supported(torch.zeros(4, 2), torch.zeros(8, 2), None) is False  # (CPU: not supported, and no error)
    assert tl.wgrad_supported(torch.zeros(8192, 32), 32) is False


def test_bf16_linear_flag_needs_bf16():
    from sparsefactorization_amd import psf_training, token_linear as tl
    with pytest.raises(SystemExit) as e:
        psf_training.main(["--problem", "adding", "--bf16-linear"])
    assert "--bf16-linear needs --bf16" in str(e.value)
    with pytest.raises(SystemExit) as e:
        psf_training.main(["--problem", "adding", "--bf16"])
    assert "--bf16 needs --problem order" in str(e.value)
    assert tl.bf16_linear_route == "never"  # neither exit touched the switch


@pytest.mark.parametrize("route", ["never", "always"])
def test_cpu_and_autocast_operands_take_the_stock_module(monkeypatch, route):
    from sparsefactorization_amd import _lib, token_linear as tl
    monkeypatch.setattr(tl, "bf16_linear_route", route)
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was reached")))
    torch.manual_seed(0)
    for fin, fout in ((2, 32), (32, 8)):
        mine, stock = tl.TokenLinear(fin, fout).to(BF16), nn.Linear(fin, fout).to(BF16)
        stock.load_state_dict(mine.state_dict())
        x = torch.randn(4, 1024, fin).to(BF16)  # T = 4096: at the kernel's gate, but on the CPU
        assert not tl.wgrad_supported(x.reshape(-1, fin), fout) and not tl.affine_rows_supported(x, mine.weight, mine.bias)
        for amp in (False, True):
            xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            with torch.autocast("cpu", dtype=BF16, enabled=amp):
                ya, yb = mine(xa), stock(xb)
            assert torch.equal(ya, yb)
            ya.float().square().sum().backward()
            yb.float().square().sum().backward()
            assert torch.equal(xa.grad, xb.grad) and torch.equal(mine.weight.grad, stock.weight.grad) and torch.equal(mine.bias.grad, stock.bias.grad)
            mine.zero_grad(), stock.zero_grad()
        with torch.no_grad():
            assert torch.equal(mine(x), stock(x))


def test_linear_wgrad_type_errors_name_the_operand(monkeypatch):
    from sparsefactorization_amd import token_linear as tl
    xb, xf = torch.zeros(4096, 8, dtype=BF16), torch.zeros(4096, 8)
    with pytest.raises(TypeError, match=r"takes float32 .*; x is torch\.bfloat16"):
        tl.linear_wgrad(xb, xb)  # "never": bf16 is a foreign dtype
    with pytest.raises(TypeError, match=r"takes float32 .*; dy is torch\.bfloat16"):
        tl.linear_wgrad(xf, xb)
    monkeypatch.setattr(tl, "bf16_linear_route", "always")
    with pytest.raises(TypeError, match=r"takes bfloat16 .*; dy is torch\.float32"):
        tl.linear_wgrad(xb, xf)
    with pytest.raises(TypeError, match=r"takes float32 .*; dy is torch\.bfloat16"):
        tl.linear_wgrad(xf, xb)
    with pytest.raises(TypeError, match=r"takes float32 .*; x is torch\.float64"):
        tl.linear_wgrad(xf.double(), xf)
    with pytest.raises(TypeError, match=r"takes float32 .*; dy is <class 'NoneType'>"):
        tl.linear_wgrad(xf, None)
    with pytest.raises(TypeError, match=r"takes bfloat16 .*; x is on 'cpu'"):
        tl.linear_wgrad(xb, xb)  # the right dtype at "always", the wrong device


C99_CONSUMER = r"""
#include <stdio.h>
#include "psf_chord.h"
#include "psf_chord_tuning.h"

typedef int64_t (*ws_fn)(int64_t, int32_t, int32_t);
typedef int (*wgrad_fn)(const uint16_t*, int64_t, const uint16_t*, int64_t, int64_t, int32_t, int32_t, uint16_t*, uint16_t*, void*,
                        int64_t, void*);
typedef int (*rows_fn)(const uint16_t*, const uint16_t*, const uint16_t*, uint16_t*, int64_t, int32_t, int32_t, void*);

int main(void) {
  ws_fn ws = psf_linear_wgrad_bf16_workspace;
  wgrad_fn wgrad = psf_linear_wgrad_bf16;
  rows_fn rows = psf_affine_rows_bf16;
  static uint32_t store[8];
  static float scratch[16];
  const uint16_t* x = (const uint16_t*)store; /* 4-byte aligned: what a row stride of 2 asks for */
  uint16_t out[8];
  int a = wgrad(NULL, 2, x, 2, 4, 2, 2, out, NULL, scratch, 64, NULL);
  int b = wgrad(x, 2, x, 2, 0, 2, 2, out, NULL, scratch, 64, NULL);
  int c = wgrad(x, 1, x, 2, 4, 2, 2, out, NULL, scratch, 64, NULL);
  int d = wgrad(x, 2, x, 2, 4, 2, 2, out, NULL, scratch, 4, NULL);
  int e = rows(NULL, x, NULL, out, 4, 2, 8, NULL);
  int f = rows(x, x, NULL, out, 4, 4, 8, NULL);
  printf("ws=%lld none=%lld codes=%d,%d,%d,%d,%d,%d\n", (long long)ws(70001, 32, 32), (long long)ws(1, 129, 1), a, b, c, d, e, f);
  return 0;
}
"""


def test_header_is_c99_with_the_new_declarations(lib, tmp_path):
    from sparsefactorization_amd import build
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "consumer.c"
    src.write_text(C99_CONSUMER)
    exe = tmp_path / "consumer"
    libdir = os.path.dirname(build.LIB_PATH)
    cmd = [gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
           "-L", libdir, "-l:libpsf_chord.so", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, f"consumer exited {run.returncode}: {run.stdout} {run.stderr}"
    want = C.plan(70001, 32, 32)["workspace_bytes"]
    assert run.stdout.strip() == f"ws={want} none=-1 codes=-1,-2,-2,-2,-1,-2"


def test_workspace_query_is_the_mirrored_plan(lib):
    for T, m, n in ((1, 1, 1), (4096, 2, 32), (4097, 127, 128), (70001, 32, 32), (70001, 128, 128), (40 * 16384, 128, 128)):
        assert lib.psf_linear_wgrad_bf16_workspace(T, m, n) == C.plan(T, m, n)["workspace_bytes"], (T, m, n)
    for T, m, n in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 129, 1), (1, 1, 129)):
        assert lib.psf_linear_wgrad_bf16_workspace(T, m, n) == -1

"""CPU: build.kernel_resources reads the code-object metadata hipcc writes at the end of a gfx950 assembly file — the check that
the bf16 producer backward uses no scratch memory rests on it (build.NO_SCRATCH_UNITS)."""
import pytest

from sparsefactorization_amd import build

METADATA = """\
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           2904
        .value_kind:     by_value
        .name:           not_a_kernel
    .group_segment_fixed_size: 110848
    .kernarg_segment_align: 8
    .name:           _ZN12_GLOBAL__N_114mlp_bwd_bf16_kILi2EEEvNS_6BwArgsE
    .private_segment_fixed_size: 0
    .sgpr_count:     60
    .symbol:         _ZN12_GLOBAL__N_114mlp_bwd_bf16_kILi2EEEvNS_6BwArgsE.kd
    .vgpr_count:     214
    .vgpr_spill_count: 0
  - .agpr_count:     4
    .args:           []
    .group_segment_fixed_size: 0
    .name:           spilling_k
    .private_segment_fixed_size: 264
    .symbol:         spilling_k.kd
    .vgpr_count:     256
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
"""


def test_kernel_resources_reads_each_kernels_entry(tmp_path):
    path = tmp_path / "unit.s"
    path.write_text("\ts_endpgm\n" + METADATA)
    res = build.kernel_resources(str(path))
    assert res == {
        "_ZN12_GLOBAL__N_114mlp_bwd_bf16_kILi2EEEvNS_6BwArgsE": {"agpr": 0, "lds": 110848, "private_segment": 0, "vgpr": 214},
        "spilling_k": {"agpr": 4, "lds": 0, "private_segment": 264, "vgpr": 256},
    }


def test_no_metadata_reads_as_no_kernels(tmp_path):
    path = tmp_path / "unit.s"
    path.write_text("\ts_endpgm\n")
    assert build.kernel_resources(str(path)) == {}


def test_a_spill_or_an_unreadable_file_fails_the_unit(tmp_path):
    good = tmp_path / "good.s"
    good.write_text(METADATA.split("  - .agpr_count:     4")[0])
    build.check_no_scratch("mlp_bwd_bf16", str(good))
    bad = tmp_path / "bad.s"
    bad.write_text(METADATA)
    with pytest.raises(RuntimeError, match="spilling_k"):
        build.check_no_scratch("mlp_bwd_bf16", str(bad))
    empty = tmp_path / "empty.s"
    empty.write_text("\ts_endpgm\n")
    with pytest.raises(RuntimeError, match="none found"):
        build.check_no_scratch("mlp_bwd_bf16", str(empty))


def test_the_unit_is_on_the_list():
    assert "mlp_bwd_bf16" in build.NO_SCRATCH_UNITS

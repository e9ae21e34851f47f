"""`gpu` tier of the fused head-and-loss kernels: the checks of test_head_emulated.py through the C ABI of libatomai_amd.so
on a real MI355X, plus engine.PxLossNode itself through a whole net at a geometry beyond one tile."""
import pytest
import torch

import _head_checks as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _require_gpu_and_native_lib():
    assert torch.cuda.is_available(), "gpu tier needs an MI355X"
    from atomai_amd import _lib
    _lib.load()                                   # raises if the HIP extension is missing
    assert not _lib.is_test_backend()
    maps = open("/proc/self/maps").read()
    assert "libatomai_amd.so" in maps, "native library not mapped"
    hips = {l.split()[-1] for l in maps.splitlines() if "libamdhip64" in l}
    assert len(hips) == 1, f"more than one HIP runtime mapped: {hips}"


@pytest.mark.parametrize("name", list(C.CASES))
def test_fused_head_vs_fp64(name):
    C.check_case(name, "cuda")


@pytest.mark.parametrize("fn,why", C.REFUSALS)
def test_bad_arguments_are_refused_before_any_launch(fn, why):
    C.check_refusal(fn, why, "cuda")


def test_scale_unless_one_multi():
    C.check_scale_unless_one_multi("cuda")


@pytest.mark.parametrize("kind", ["ce", "dice"])
def test_net_head_beyond_one_tile_equals_the_modular_path(kind):
    C.check_net_beyond_one_tile("cuda", kind)

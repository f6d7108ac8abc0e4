"""CPU tests of downsample_point_cloud_poisson_disk (src/sample_point_cloud.cpp:253-333 in the reference): the reference's error texts and
the input checks are made on the host before any device work; without a GPU the call raises instead of computing on the CPU; the C entry
points are declared in include/pcu_hip.h (tests/test_abi.py then also checks that the library exports them)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to reach the device (a context) fails the test."""
    from point_cloud_utils_amd import _lib

    def _touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "ctx", _touched)


def test_exported_from_the_package():
    import point_cloud_utils_amd as pcu
    assert "downsample_point_cloud_poisson_disk" in pcu.__all__
    assert callable(pcu.downsample_point_cloud_poisson_disk)


def test_reference_error_texts(no_device):
    import point_cloud_utils_amd as pcu
    v = np.random.default_rng(0).random((100, 3))
    with pytest.raises(ValueError, match=re.escape("Cannot have both num_samples <= 0 and radius <= 0")):
        pcu.downsample_point_cloud_poisson_disk(v, 0.0)
    with pytest.raises(ValueError, match=re.escape("Cannot have both num_samples <= 0 and radius <= 0")):
        pcu.downsample_point_cloud_poisson_disk(v, -1.0, target_num_samples=0)
    for tol in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match=re.escape("sample_num_tolerance must be in (0, 1]")):
            pcu.downsample_point_cloud_poisson_disk(v, 0.1, sample_num_tolerance=tol)


def test_zero_rows_and_non_finite_input_refused_on_the_host(no_device):
    import point_cloud_utils_amd as pcu
    for dt in (np.float32, np.float64):
        with pytest.raises(ValueError, match="zero elements"):
            pcu.downsample_point_cloud_poisson_disk(np.zeros((0, 3), dtype=dt), 0.1)
        with pytest.raises(ValueError, match="zero elements"):
            pcu.downsample_point_cloud_poisson_disk(np.zeros((0, 3), dtype=dt), 0.0, target_num_samples=10)
        for bad in (np.nan, np.inf, -np.inf):
            v = np.random.default_rng(1).random((50, 3)).astype(dt)
            v[17, 1] = bad
            with pytest.raises(ValueError, match="NaN or infinite"):
                pcu.downsample_point_cloud_poisson_disk(v, 0.1)
            with pytest.raises(ValueError, match="NaN or infinite"):
                pcu.downsample_point_cloud_poisson_disk(v, 0.0, target_num_samples=10)


def test_dtype_shape_and_seed_checks(no_device):
    import point_cloud_utils_amd as pcu
    with pytest.raises(ValueError, match="Invalid scalar type"):
        pcu.downsample_point_cloud_poisson_disk(np.zeros((10, 3), dtype=np.int32), 0.1)
    with pytest.raises(ValueError, match=r"shape \(n, 3\)"):
        pcu.downsample_point_cloud_poisson_disk(np.zeros((10, 2)), 0.1)
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        pcu.downsample_point_cloud_poisson_disk(np.zeros((10, 3)), 0.1, random_seed=-1)
    with pytest.raises(ValueError, match="NaN"):
        pcu.downsample_point_cloud_poisson_disk(np.zeros((10, 3)), float("nan"))


def test_no_cpu_fallback_without_gpu():
    import point_cloud_utils_amd as pcu
    from point_cloud_utils_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("GPU present")
    v = np.random.default_rng(2).random((100, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pcu.downsample_point_cloud_poisson_disk(v, 0.1, random_seed=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pcu.downsample_point_cloud_poisson_disk(v, 0.0, target_num_samples=1000)      # (target >= n: all rows, still on the device)


def test_entry_points_declared_in_the_header():
    src = open(os.path.join(ROOT, "include", "pcu_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for suf in ("f32", "f64"):
        assert re.search(r"\bint pcu_hip_poisson_disk_%s\s*\(" % suf, src)
    from point_cloud_utils_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "pcu_hip_poisson_disk_f32") and hasattr(L, "pcu_hip_poisson_disk_f64")

"""cancel() from a second thread during segment_point_cloud_plane, and the context's answers afterwards (-m gpu). Modelled on
tests/test_gpu_zz_icp_cancel.py, with its bound. A file of its own that sorts last, as that one is: an abandoned call makes every context
reset its cross-call state, and the end-to-end Chamfer comparison of tests/test_gpu_mesh_sampling.py fails by one ulp when such a reset happens
in a file before it (Tests)."""
import threading
import time

import numpy as np
import pytest

import plane_contract as pc
from test_gpu_point_cloud_plane import same
from test_plane_contract import planted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def test_cancel_from_another_thread(pcu):
    """A canceller thread asks every 5 ms until the main thread has left its call. The call in flight tests 2^22 rows against 2^20 hypotheses:
    2^42 tests of 8 float64 operations, 0.45 s at the chip's peak vector float64 rate (78.6 TFLOP/s, the figure of
    profiles/plane_record.json) and several times that measured -- it is scored in 256 launches, at most two in the queue, and ends with
    KeyboardInterrupt between two of them. Afterwards the context answers a small call with the contract's bytes."""
    import torch
    rng = np.random.default_rng(16)
    cloud = torch.from_numpy(rng.random((1 << 22, 3), dtype=np.float32)).cuda()
    started, done = threading.Event(), threading.Event()

    def canceller():
        started.wait()
        for _ in range(2000):
            time.sleep(0.005)
            pcu.cancel()
            if done.is_set():
                break
    th = threading.Thread(target=canceller); th.start()
    t0 = time.perf_counter()
    try:
        with pytest.raises(KeyboardInterrupt):
            started.set()
            pcu.segment_point_cloud_plane(cloud, 0.01, 2 ** 20, 1)
    finally:
        done.set(); th.join()
    assert time.perf_counter() - t0 < 60.0
    P = planted(4097, np.float32)
    for refit in (False, True):
        want = pc.segment_plane(P, 0.01, 128, 3, refit=refit)
        same(pcu.segment_point_cloud_plane(P, 0.01, 128, 3, refit), want, P)
        T = torch.from_numpy(P).cuda()
        same(pcu.segment_point_cloud_plane(T, 0.01, 128, 3, refit), want, T)

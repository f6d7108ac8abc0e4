"""cancel() from a second thread during cluster_point_cloud_dbscan, and the context's answers afterwards (-m gpu). Shaped after
test_cancel_from_another_thread of tests/test_gpu_radius.py, with its bound. A file of its own that sorts last, as
tests/test_gpu_zz_fps_cancel.py is: an abandoned call makes every context reset its cross-call state, and the end-to-end Chamfer comparison of
tests/test_gpu_mesh_sampling.py fails by one ulp when such a reset happens in a file before it (Tests)."""
import threading
import time

import numpy as np
import pytest

import dbscan_contract as dc
from test_gpu_point_cloud_dbscan import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def test_cancel_from_another_thread(pcu):
    """Shaped after tests/test_gpu_radius.py: a canceller thread asks until the main thread has left its loop of calls; the call in flight
    ends with KeyboardInterrupt, and the context answers as before. With more min_points than rows the core pass never stops early."""
    import torch
    p = torch.from_numpy(np.random.default_rng(15).random((1 << 19, 3), dtype=np.float32)).cuda()
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
            for _ in range(400):                                           # (every call walks 2^38 pairs)
                pcu.cluster_point_cloud_dbscan(p, 2.0, 1 << 20)
    finally:
        done.set(); th.join()
    assert time.perf_counter() - t0 < 60.0
    a = p[:3000].cpu().numpy()
    want = dc.dbscan(a, 0.05, 3)
    same(pcu.cluster_point_cloud_dbscan(a, 0.05, 3, return_core=True), want)
    same(pcu.cluster_point_cloud_dbscan(p[:3000], 0.05, 3, return_core=True), want)

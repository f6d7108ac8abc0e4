"""cancel() from a second thread during register_point_clouds_icp, and the context's answers afterwards (-m gpu). Modelled on
tests/test_gpu_zz_dbscan_cancel.py, with its bound. A file of its own that sorts last, as that one is: an abandoned call makes every context
reset its cross-call state, and the end-to-end Chamfer comparison of tests/test_gpu_mesh_sampling.py fails by one ulp when such a reset happens
in a file before it (Tests)."""
import threading
import time

import numpy as np
import pytest

import icp_contract as ic
from test_gpu_point_cloud_icp import pair, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def test_cancel_from_another_thread(pcu):
    """A canceller thread asks until the main thread has left its call; the registration in flight -- a million points, tolerances of zero so
    that it never converges, more iterations than anybody waits for -- ends with KeyboardInterrupt between two evaluations or inside a search,
    and the context answers as before."""
    import torch
    rng = np.random.default_rng(15)
    tgt = torch.from_numpy(rng.random((1 << 20, 3), dtype=np.float32)).cuda()
    src = torch.from_numpy(rng.random((1 << 20, 3), dtype=np.float32)).cuda()
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
            pcu.register_point_clouds_icp(src, tgt, max_iterations=10 ** 6, relative_fitness=0.0, relative_rmse=0.0)
    finally:
        done.set(); th.join()
    assert time.perf_counter() - t0 < 60.0
    s, t, nrm = pair(3000, 2500, np.float32)
    want = ic.register_icp(s, t, nrm, return_correspondences=True, nearest=lambda p, q: pcu.k_nearest_neighbors(p, q, 1, squared_distances=True))
    same(pcu.register_point_clouds_icp(s, t, nrm, return_correspondences=True), want, s)
    ts, tt, tn = (torch.from_numpy(a).cuda() for a in (s, t, nrm))
    same(pcu.register_point_clouds_icp(ts, tt, tn, return_correspondences=True), want, ts)

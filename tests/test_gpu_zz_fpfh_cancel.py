"""cancel() from a second thread during compute_point_cloud_fpfh, and the context's answers afterwards (-m gpu). Shaped after
tests/test_gpu_zz_dbscan_cancel.py, with its bound. A file of its own that sorts last, for that file's reason: an abandoned call makes every
context reset its cross-call state, and the end-to-end Chamfer comparison of tests/test_gpu_mesh_sampling.py fails by one ulp when such a
reset happens in a file before it (Tests)."""
import threading
import time

import numpy as np
import pytest

import fpfh_contract as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def test_cancel_from_another_thread(pcu):
    """A canceller thread asks until the main thread has left its loop of calls; the call in flight ends with KeyboardInterrupt, and the context
    answers as before. With a radius that holds the cloud every call computes 2^32 pairs: one cell, so only the polls inside a run of records
    can see the request."""
    import torch
    rng = np.random.default_rng(16)
    p = torch.from_numpy(rng.random((1 << 16, 3), dtype=np.float32)).cuda()
    nrm = torch.from_numpy(rng.standard_normal((1 << 16, 3)).astype(np.float32)).cuda()
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
            for _ in range(400):
                pcu.compute_point_cloud_fpfh(p, nrm, 2.0)
    finally:
        done.set(); th.join()
    assert time.perf_counter() - t0 < 60.0
    a, an = p[:1000].cpu().numpy(), nrm[:1000].cpu().numpy()
    want_f, want_c, m = fc.fpfh(a, an, 0.15)
    for kind in ((a, an), (p[:1000], nrm[:1000])):
        f, c = pcu.compute_point_cloud_fpfh(*kind, 0.15, return_spfh=True)
        f, c = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in (f, c))
        assert np.array_equal(c, want_c)
        assert (np.abs(f - want_f) <= np.spacing(np.maximum(np.abs(f), np.abs(want_f)))).all()

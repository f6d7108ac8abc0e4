"""cancel() from a second thread during register_point_clouds_ransac, and the context's answers afterwards (-m gpu). Modelled on
tests/test_gpu_zz_plane_cancel.py, with its bound. A file of its own that sorts last, as that one is: an abandoned call makes every context
reset its cross-call state, and the end-to-end Chamfer comparison of tests/test_gpu_mesh_sampling.py fails by one ulp when such a reset happens
in a file before it (Tests)."""
import threading
import time

import numpy as np
import pytest

import ransac_contract as rc
from test_gpu_point_cloud_ransac import same
from test_ransac_contract import THR, planted

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcu():
    import point_cloud_utils_amd as m
    from point_cloud_utils_amd import _lib
    assert _lib.device_count() > 0, "no GPU visible: the gfx950 path has no CPU fallback"
    return m


def test_cancel_from_another_thread(pcu):
    """A canceller thread asks every 5 ms until the main thread has left its call. The call in flight tests 2^20 correspondences against 2^20
    hypotheses (the edge pre-check off, so that every hypothesis is scored in full): 2^40 tests of 26 float64 operations, 0.36 s at the chip's
    peak vector float64 rate (78.6 TFLOP/s, the figure of profiles/plane_record.json) and several times that measured -- it is scored in 64
    launches, at most two in the queue, and ends with KeyboardInterrupt between two of them. Afterwards the context answers a small call with
    the contract's bytes."""
    import torch
    rng = np.random.default_rng(16)
    c = 1 << 20
    source = torch.from_numpy(rng.random((c, 3), dtype=np.float32)).cuda()
    target = torch.from_numpy(rng.random((c, 3), dtype=np.float32)).cuda()
    corr = torch.from_numpy(np.ascontiguousarray(np.stack([np.arange(c), rng.permutation(c)], axis=1).astype(np.int64))).cuda()
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
            pcu.register_point_clouds_ransac(source, target, corr, 0.01, 2 ** 20, 1, edge_length_ratio=0.0)
    finally:
        done.set(); th.join()
    assert time.perf_counter() - t0 < 60.0
    P = planted(1000, np.float32)
    for refit in (False, True):
        want = rc.register_ransac(P.source, P.target, P.corr, THR, 128, 3, refit=refit)
        same(pcu.register_point_clouds_ransac(P.source, P.target, P.corr, THR, 128, 3, refit=refit), want, P.source)
        A = tuple(torch.from_numpy(x).cuda() for x in (P.source, P.target, P.corr))
        same(pcu.register_point_clouds_ransac(*A, THR, 128, 3, refit=refit), want, A[0])

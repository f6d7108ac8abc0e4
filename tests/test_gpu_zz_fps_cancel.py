"""Cancellation of a long farthest-point sampling (-m gpu), after tests/test_gpu_cancel.py's method. A file of its own that sorts behind the
other GPU files on purpose: an abandoned call makes every context reset the state it keeps between calls (the fill words of the one-pass
index build, the grid layout handed down between two-sided calls), and tests/test_gpu_mesh_sampling.py's end-to-end Chamfer comparison of
device against host input is bit-exact only for the state the files before it leave."""
import threading
import time

import numpy as np
import pytest

from test_gpu_fps import check, make, pcu, reference, same  # noqa: F401  (pcu: the module fixture)

pytestmark = pytest.mark.gpu


def test_cancel_from_another_thread(pcu):
    """A canceller thread asks until the main thread has left its loop of long samplings (2^20 points, 2^17 samples: thousands of graph
    replays each): the call in flight ends with KeyboardInterrupt between two replays, and the context answers as before. Shaped after
    tests/test_gpu_cancel.py."""
    import torch
    p = torch.from_numpy(np.random.default_rng(21).random((1 << 20, 3), dtype=np.float32)).cuda()
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
                pcu.downsample_point_cloud_farthest_point(p, 1 << 17)
    finally:
        done.set(); th.join()
    assert time.perf_counter() - t0 < 60.0
    check("uniform70001", np.float32, 70001, 5, 65)
    check("uniform70001", np.float64, 3000, 5, 65)
    host = make("uniform70001", np.float32)[:40000]
    got = pcu.downsample_point_cloud_farthest_point(torch.from_numpy(host.copy()).cuda(), 70, 9, return_distances=True)
    same((got[0].cpu().numpy(), got[1].cpu().numpy()), *reference("uniform70001", "float32", 40000, 9, 70)[::2])

"""A handle's teardown frees everything it allocated on the device: aos_ctx::release() keeps only what has an order
(threads, streams, events), and every device buffer goes with its owning member when aos_destroy deletes the handle.

Ten cycles in one process, each through every owner of device memory the GVD stage has (the seed-gen frame, the
synchronous GVD with the markers' worker, an external GVD, a pipelined lane whose job is still in flight when the
handle is closed). Free device memory is read after cycle 2 (the runtime's own pools are warm by then) and after cycle
10: what a cycle loses is lost eight times in between.

The bound is measured, not chosen: the parent commit, whose release() listed its buffers by hand, drops
PARENT_DROP bytes over the same cycles; one allocation granule of the runtime (the step by which free memory moves for
a 256-byte hipMalloc, observed in that run and printed again here) is the margin. The runtime hands small blocks out
of 2 MiB granules, so free memory shows a loss once it fills a granule: eight cycles show one of 256 KiB per handle,
not a single lost 256-byte scalar."""
import ctypes

import pytest

import aos_gpu
import gvd_scenes as GS
import shapes as S

pytestmark = pytest.mark.gpu

CYCLES = 10
PARENT_DROP = 0            # bytes, the parent commit over cycles 3-10 of this test body
GRANULE = 2 * 1024 * 1024  # bytes, the first step of free memory under 256-byte hipMallocs in the same run


def alloc_granule(limit=16384):
    """The step by which free device memory first moves while 256-byte blocks are allocated (0: it never moved)."""
    import torch
    L = aos_gpu.lib()   # (the HIP runtime the library is bound to)
    L.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    L.hipFree.argtypes = [ctypes.c_void_p]
    free0, step, blocks = torch.cuda.mem_get_info()[0], 0, []
    for _ in range(limit):
        p = ctypes.c_void_p()
        assert L.hipMalloc(ctypes.byref(p), 256) == 0
        blocks.append(p)
        step = free0 - torch.cuda.mem_get_info()[0]
        if step:
            break
    for p in blocks:
        assert L.hipFree(p) == 0
    return step


def one_cycle(frame, lattice):
    cloud, poly, akw = frame
    c = aos_gpu.Ctx(aos_gpu.default_params(gvd_markers=1, **akw))
    c.set_polygon(poly)
    c.seedgen(cloud)
    c.gvd_from_seedgen()
    c.gvd(*lattice)
    c.gvd_async()
    c.close()   # (the pipelined job is still in flight, or just done: release() joins it either way)


def test_ten_handles_leave_no_device_memory_behind():
    import torch
    W, H, R = min(S.GRID_CASES, key=lambda c: c[0] * c[1])
    cloud, poly, akw, _ = S.scene(S.border_pattern(W, H, S.grid_case_seed(W, H, R)), R)
    assert akw["grid_resolution"] == GS.RES
    frame, lattice = (cloud, poly, akw), GS.scene("lattice")
    torch.cuda.mem_get_info()
    free = []
    for k in range(CYCLES):
        one_cycle(frame, lattice)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    drop = free[1] - free[CYCLES - 1]
    print(f"free after each cycle, relative to cycle 2: {[f - free[1] for f in free]}; drop over cycles 3-{CYCLES}: "
          f"{drop} bytes; a 256-byte hipMalloc moves free memory by {alloc_granule()} bytes here")
    assert drop <= PARENT_DROP + GRANULE, (drop, free)

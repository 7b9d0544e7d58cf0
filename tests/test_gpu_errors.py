"""GPU error paths: a frame that fails after finish_frame (thinning that does not converge within the
launch cap) must not be served afterwards (have_frame was set before the deferred checks).
"""
import pytest

import aos_gpu
import orchard

pytestmark = pytest.mark.gpu


def test_failed_frame_is_not_served():
    cfg = orchard.CONFIGS["C1"]   # T ~ 13 at 0.1 m: more than one temporal block of 8 iterations
    cloud = orchard.generate(cfg)
    ctx = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res))
    ctx.set_polygon(orchard.polygon(cfg))
    good = ctx.seedgen(cloud)   # a good frame first: the state the failure must clear
    assert good["thin_iters"] > 8
    gg = ctx.gvd_from_seedgen()
    assert len(gg["nodes"]) > 0
    aos_gpu.debug_limits(thin_cap=1)   # one launch: thinning cannot converge
    try:
        with pytest.raises(RuntimeError, match="did not converge"):
            ctx.seedgen(cloud)
        for call in (ctx.gvd_from_seedgen, ctx.gvd_async):
            with pytest.raises(RuntimeError, match="no seed-gen frame"):
                call()
        with pytest.raises(RuntimeError, match="no frame"):
            ctx.debug_grid("raster", (good["height"], good["width"]))
    finally:
        aos_gpu.debug_limits()
    # the handle recovers on the next good frame, which also shows that the cap is back at its default
    again = ctx.seedgen(cloud)
    assert again["thin_iters"] == good["thin_iters"]
    assert len(ctx.gvd_from_seedgen()["nodes"]) == len(gg["nodes"])
    ctx.close()

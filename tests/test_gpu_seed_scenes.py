"""The row, ray and seed kernels (assemble_rows, k_virtual_candidates with d_raycast, k_endpoint_rays, the three first-come
0.5 m de-duplications, k_concat3: the second half of run_cluster_seed_stage) on the designed skeletons of
tests/seed_scenes.py, bit for bit against the oracle. Every scene's regime is asserted on the oracle and the numpy
reference before the frame runs (seed_scenes.oracle_frame; tests/test_seed_scenes_cpu.py does the same without a GPU),
so a scene that has drifted out of the branch it is meant for fails instead of passing vacuously."""
import pytest

import aos_gpu
import aos_tiles as T
import seed_scenes as SS
from parity_util import assert_gvd_parity, assert_seedgen_parity, assert_seeds_exact

pytestmark = pytest.mark.gpu


def check_frame(ctx, g, name):
    f, o, ref, fig, og, _ = SS.oracle_frame(name)
    assert_seeds_exact(g, o)
    assert_seedgen_parity(g, o)
    assert g["n_clipped"] == o["n_clipped"]
    if og is not None:
        assert_gvd_parity(ctx.gvd_from_seedgen(), og)


def run_frame(ctx, name):
    f = SS.oracle_frame(name)[0]
    ctx.set_polygon(f["polygon"])
    g = ctx.seedgen(f["cloud"])
    check_frame(ctx, g, name)
    return g


def new_ctx(name):
    return aos_gpu.Ctx(aos_gpu.default_params(**SS.oracle_frame(name)[0]["akw"]))


@pytest.mark.parametrize("name", list(SS.SCENES))
def test_scene_vs_oracle(name):
    c = new_ctx(name)
    try:
        run_frame(c, name)
    finally:
        c.close()


def test_one_handle_through_changing_grids():
    """A wide grid, a square one, a small one whose rows have no slots, the wide one again: the distance table of
    k_endpoint_rays is rebuilt for every new grid diagonal (longer, shorter, longer), the candidate and seed buffers
    are reused while the frames shrink, the virtual count is cleared by the memset branch."""
    kw = [SS.oracle_frame(n)[0]["akw"] for n in SS.HANDLE_ORDER]
    assert all(k == kw[0] for k in kw), "one handle: the frames must share their parameters"
    c = new_ctx(SS.HANDLE_ORDER[0])
    try:
        for k, name in enumerate(SS.HANDLE_ORDER):
            try:
                run_frame(c, name)
            except AssertionError as e:
                raise AssertionError(f"frame {k} ({name}) after {SS.HANDLE_ORDER[:k]}: {e}") from e
    finally:
        c.close()


@pytest.mark.parametrize("tiles", [(2, 2), (3, 1)], ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("name", SS.TILED_SCENES)
def test_scene_tiled_vs_oracle(name, tiles):
    """The same frames through aos_group_* (ranks as the library's threads on one GPU, root = the last rank): the rows
    then come from cluster_dist.hip's records."""
    f = SS.oracle_frame(name)[0]
    world = tiles[0] * tiles[1]
    root = world - 1
    grp = aos_gpu.Group(aos_gpu.default_params(**f["akw"]), [0] * world, *tiles)
    try:
        grp.set_polygon(f["polygon"])
        parts = [T.shard(f["cloud"], grp.plan(r)["points_box"]) for r in range(world)]
        g = grp.process(parts, root=root)
        check_frame(grp.rank(root), g, name)
    finally:
        grp.close()

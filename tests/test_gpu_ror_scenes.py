"""csrc/ror.hip and csrc/ror_stage.hip on the designed clouds of tests/ror_scenes.py: the raw raster
(debug_grid) bit for bit, n_clipped, n_input and n_ror_read against the oracle, then the rest of the frame. Each scene
forces a compare rule or a branch that orchard clouds reach by accident at best; tests/test_ror_scenes_cpu.py asserts,
without a GPU, that it does and that the oracle equals an independent numpy reference on it."""
import functools

import numpy as np
import pytest

import aos_gpu
import oracle_py as O
import ror_scenes as RS
from parity_util import assert_seedgen_parity, binned_box, inside

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def oracle(name, dense):
    sc = RS.scene(name)
    return O.seedgen(sc.cloud, sc.polygon, O.default_params(**RS.oracle_kwargs(sc.akw)), is_dense=dense)


def new_ctx(sc):
    c = aos_gpu.Ctx(aos_gpu.default_params(**sc.akw))
    if sc.polygon is not None:
        c.set_polygon(sc.polygon)
    return c


def check_frame(c, g, o, sc, xyz, dense, what, n_read=None):
    """g: the GPU frame of the points xyz (a scene's, or a prefix of them), o: the oracle's."""
    H, W = o["height"], o["width"]
    assert (g["width"], g["height"]) == (W, H), what
    raster = c.debug_grid("raster", (H, W)) != 0
    want = o["raster"] != 0
    if not np.array_equal(raster, want):
        ref = RS.reference(xyz, sc.polygon, sc.akw, dense)
        ys, xs = np.nonzero(raster != want)
        bad = [i for i in np.flatnonzero(ref["cand"]) if (ref["gy"][i], ref["gx"][i]) in set(zip(ys, xs))]
        sub = RS.Scene(sc.name, xyz, sc.polygon, sc.akw, [])
        first = RS.describe(sub, ref, dense, int(bad[0])) if bad else f"cell ({xs[0]}, {ys[0]}) holds no candidate"
        raise AssertionError(f"{what}: raster differs in {len(ys)} cells (GPU set {int(raster[ys, xs].sum())} of them); "
                             f"first: {first}")
    assert g["n_clipped"] == o["n_clipped"], (what, g["n_clipped"], o["n_clipped"])
    assert g["n_input"] == o["n_input"] == len(xyz), what
    if n_read is not None:
        assert g["n_ror_read"] == n_read, (what, g["n_ror_read"], n_read)
    assert_seedgen_parity(g, o)


def box_count(sc, xyz):
    """The points a host cloud's split upload leaves for the partition passes: those inside the binned box."""
    poly = RS.DEFAULT_POLYGON if sc.polygon is None else np.asarray(sc.polygon)
    box = binned_box(poly, sc.akw["ror_radius"], sc.akw["clipping_minz"], sc.akw["clipping_maxz"])
    return inside(RS.as_cloud(xyz), box)


@pytest.mark.parametrize("name", [n for n in RS.SCENES if n != "layouts"])
def test_scene_on_a_fresh_handle(name):
    """A host cloud (the split upload: only the binned box's points are read), each mode on a fresh handle."""
    sc = RS.scene(name)
    for dense in sc.modes:
        c = new_ctx(sc)
        g = c.seedgen(sc.cloud, is_dense=dense)
        check_frame(c, g, oracle(name, dense), sc, sc.xyz, dense, f"{name} dense={dense}", box_count(sc, sc.xyz))
        c.close()


def test_big_tiles_twice_on_one_handle():
    """The first frame finds its big tiles without the big-tile kernels and is redone; the second launches them."""
    sc = RS.scene("big_tiles")
    c = new_ctx(sc)
    for k in range(2):
        g = c.seedgen(sc.cloud, is_dense=True)
        check_frame(c, g, oracle("big_tiles", True), sc, sc.xyz, True, f"big_tiles frame {k}", box_count(sc, sc.xyz))
    c.close()


@pytest.mark.parametrize("what,step,offs", RS.LAYOUTS)
def test_layouts(what, step, offs):
    import torch
    sc = RS.scene("layouts")
    c = new_ctx(sc)
    if what == "host":
        g = c.seedgen(sc.cloud, is_dense=False)
        n_read = box_count(sc, sc.xyz)
    else:
        rec = RS.relayout(sc.xyz, step, offs)
        d = torch.from_numpy(rec).to("cuda:0")
        torch.cuda.synchronize()
        g = c.seedgen(d.data_ptr(), n_points=len(rec), point_step=step, offs=offs, is_dense=False, on_device=True)
        n_read = len(rec)
    check_frame(c, g, oracle("layouts", False), sc, sc.xyz, False, f"layouts {what}", n_read)
    c.close()


@pytest.mark.parametrize("name", [n for n in RS.SCENES if n.startswith("chunk_edges")])
def test_chunk_edges_on_device(name):
    """The records stay where the scene put them (a device cloud is not split): the decisive records are the last of
    one partition chunk and the first of the next."""
    import torch
    sc = RS.scene(name)
    dense = sc.modes[0]
    d = torch.from_numpy(sc.cloud).to("cuda:0")
    torch.cuda.synchronize()
    c = new_ctx(sc)
    g = c.seedgen(d.data_ptr(), n_points=len(sc.xyz), is_dense=dense, on_device=True)
    check_frame(c, g, oracle(name, dense), sc, sc.xyz, dense, name, len(sc.xyz))
    c.close()


def test_one_handle_through_the_scenes():
    """Frames of changing size, radius, density, polygon and is_dense. A handle's parameters are fixed at creation, so
    the scenes of one parameter set share a handle; the handles run interleaved, in HANDLE_ORDER."""
    handles = {}
    try:
        for k, (name, dense) in enumerate(RS.HANDLE_ORDER):
            sc = RS.scene(name)
            key = RS.handle_key(sc)
            if key not in handles:
                handles[key] = aos_gpu.Ctx(aos_gpu.default_params(**sc.akw))
            c = handles[key]
            c.set_polygon(RS.DEFAULT_POLYGON if sc.polygon is None else sc.polygon)
            g = c.seedgen(sc.cloud, is_dense=dense)
            check_frame(c, g, oracle(name, dense), sc, sc.xyz, dense,
                        f"frame {k} ({name}, dense={dense}) after {RS.HANDLE_ORDER[:k]}", box_count(sc, sc.xyz))
    finally:
        for c in handles.values():
            c.close()


@pytest.mark.parametrize("name", RS.STREAM_SCENES)
def test_stream(name):
    """The scene delivered over four map_append calls: every frame equals the oracle on the concatenation so far."""
    sc = RS.scene(name)
    parts = RS.stream_parts(sc)
    c = new_ctx(sc)
    c.map_reset()
    for k in range(len(parts)):
        g = c.map_append(RS.as_cloud(sc.xyz[parts[k]]), is_dense=True)
        xyz = sc.xyz[np.concatenate(parts[:k + 1])]
        o = O.seedgen(RS.as_cloud(xyz), sc.polygon, O.default_params(**RS.oracle_kwargs(sc.akw)), is_dense=True)
        # (the map lives on the device: the first frame reads all of it, an append only its scan)
        check_frame(c, g, o, sc, xyz, True, f"{name} after append {k}", len(parts[k]))
    c.close()

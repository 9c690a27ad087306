"""Sparse bricked grid media on the CPU path: SparseGrid container, brick
layout vs dense layout bit-identity, NanoVDB sparse I/O, scene grammar.

The expected value of every layout comparison is the dense renderer's own
output: the two layouts load the same voxel values into the same arithmetic,
so images are compared with assert_array_equal, no tolerance."""
import hashlib
import os
import struct
import tracemalloc

import numpy as np
import pytest

import hippt
from hippt import C
from hippt.scene.nvdb import NvdbError, read_nvdb, write_nvdb
from hippt.scene.procedural import smoke_box
from hippt.scene.scene import MediumDesc, Scene
from hippt.scene.sparse_grid import SparseGrid
from hippt.scene.xml_parser import parse_xml


def random_brick_grid(shape, empty_frac=0.7, seed=11):
    """Random grid whose 8^3 bricks are empty with probability empty_frac."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    bz, by, bx = (-(-nz // 8), -(-ny // 8), -(-nx // 8))
    keep = rng.random((bz, by, bx)) >= empty_frac
    keep.flat[0] = True                       # never degenerate to all-empty
    mask = np.repeat(np.repeat(np.repeat(keep, 8, 0), 8, 1), 8, 2)[:nz, :ny, :nx]
    a = rng.random(shape).astype(np.float32) * mask
    a[rng.random(shape) < 0.3] = 0.0          # holes inside resident bricks
    return a.astype(np.float32)


def numpy_brick_count(a):
    nz, ny, nx = a.shape
    n = 0
    for z in range(0, nz, 8):
        for y in range(0, ny, 8):
            for x in range(0, nx, 8):
                n += bool(np.any(a[z:z + 8, y:y + 8, x:x + 8] != 0))
    return n


def render_cpu(desc, spp=4):
    r = hippt.PythonRenderer(desc, device_id=-1)
    img = r.render(spp=spp).numpy().copy()
    return img, r


def hand_built(density, temperature=None, width=32, height=24):
    """smoke_box geometry around a hand-built grid MediumDesc."""
    d = smoke_box(width=width, height=height, n_grid=8)
    d.media = [MediumDesc(type="grid", sigma_a=(0.3, 0.35, 0.4), sigma_s=(2.5, 2.5, 2.5),
                          phase="hg", g1=0.2, density=density, temperature=temperature,
                          emission_scale=1.5 if temperature is not None else 0.0,
                          scale=6.0, grid_lo=(-0.7, 0.05, 0.5), grid_hi=(0.7, 1.75, 1.9))]
    return d


def sparsified(desc):
    m = desc.media[0]
    m.density = SparseGrid.from_dense(m.density)
    return desc


# ------------------------------------------------------------ 1. round trip
@pytest.mark.parametrize("case", ["random", "partial", "zero", "full"])
def test_round_trip(case):
    if case == "random":
        a = random_brick_grid((17, 40, 24))
    elif case == "partial":
        a = np.arange(1, 31, dtype=np.float32).reshape(2, 3, 5)
    elif case == "zero":
        a = np.zeros((9, 8, 20), np.float32)
    else:
        a = np.random.default_rng(2).random((16, 16, 16)).astype(np.float32) + 0.5
    g = SparseGrid.from_dense(a)
    assert g.shape == a.shape
    assert g.n_bricks == numpy_brick_count(a)
    assert g.coords.dtype == np.int32 and g.coords.shape == (g.n_bricks, 3)
    assert g.values.dtype == np.float32 and g.values.shape == (g.n_bricks, 8, 8, 8)
    keys = [tuple(c) for c in g.coords]
    assert keys == sorted(set(keys))
    np.testing.assert_array_equal(g.to_dense(), a)
    assert g.dense_nbytes == a.nbytes
    assert g.nbytes == g.coords.nbytes + g.values.nbytes
    if case == "random":
        assert 0 < g.n_bricks < 3 * 5 * 3 and 0.0 < g.occupancy < 1.0
    if case == "partial":
        assert g.n_bricks == 1
        assert np.count_nonzero(g.values) == 30      # edge brick is zero-padded
    if case == "zero":
        assert g.n_bricks == 0 and g.occupancy == 0.0
    if case == "full":
        assert g.n_bricks == 8 and g.occupancy == 1.0


def test_unsorted_coords_are_sorted_and_duplicates_rejected():
    v = np.ones((2, 8, 8, 8), np.float32)
    v[1] *= 2
    g = SparseGrid((16, 8, 8), [(1, 0, 0), (0, 0, 0)], v)
    assert [tuple(c) for c in g.coords] == [(0, 0, 0), (1, 0, 0)]
    assert g.values[0, 0, 0, 0] == 2.0
    with pytest.raises(ValueError):
        SparseGrid((16, 8, 8), [(0, 0, 0), (0, 0, 0)], v)
    with pytest.raises(ValueError):
        SparseGrid((16, 8, 8), [(0, 0, 0), (2, 0, 0)], v)


# ------------------------------------------------- 2. bit-identity vs dense
@pytest.mark.parametrize("emission", [False, True])
def test_smoke_box_bricks_equal_dense(emission):
    dense, _ = render_cpu(smoke_box(width=32, height=24, n_grid=24, emission=emission))
    bricks, r = render_cpu(sparsified(smoke_box(width=32, height=24, n_grid=24,
                                                emission=emission)))
    assert r.info()["media"][0]["layout"] == "bricks"
    assert dense[..., :3].mean() > 0
    np.testing.assert_array_equal(bricks, dense)


def test_temperature_sparse_only_and_union_table():
    """A SparseGrid temperature alone switches the medium to bricks; the two
    grids share one table over the union of their bricks."""
    a = random_brick_grid((17, 40, 24), seed=5)
    t = random_brick_grid((17, 40, 24), seed=6) * 4000.0
    dense, _ = render_cpu(hand_built(a, t))
    bricks, r = render_cpu(hand_built(a, SparseGrid.from_dense(t)))
    mi = r.info()["media"][0]
    assert mi["layout"] == "bricks"
    union = numpy_brick_count(np.abs(a) + np.abs(t))
    assert mi["n_bricks"] == union > numpy_brick_count(a)
    np.testing.assert_array_equal(bricks, dense)
    with pytest.raises(ValueError):
        Scene(hand_built(SparseGrid.from_dense(a), t[:, :, :16]))


@pytest.mark.parametrize("no_super", [False, True])
def test_hand_built_bricks_equal_dense(no_super, monkeypatch):
    if no_super:
        monkeypatch.setenv("HIPPT_NO_SUPER", "1")
    a = random_brick_grid((17, 40, 24))
    dense, rd = render_cpu(hand_built(a))
    bricks, rb = render_cpu(hand_built(SparseGrid.from_dense(a)))
    sd, maj_d, avg_d = rd.scene.native.medium_super(0)
    sb, maj_b, avg_b = rb.scene.native.medium_super(0)
    assert (sd.size == 0) == no_super
    np.testing.assert_array_equal(sb, sd)         # same supergrid, cell for cell
    assert (maj_b, avg_b) == (maj_d, avg_d)
    assert dense[..., :3].mean() > 0
    np.testing.assert_array_equal(bricks, dense)


def test_smoke_box_no_super(monkeypatch):
    monkeypatch.setenv("HIPPT_NO_SUPER", "1")
    dense, _ = render_cpu(smoke_box(width=32, height=24, n_grid=24))
    bricks, _ = render_cpu(sparsified(smoke_box(width=32, height=24, n_grid=24)))
    np.testing.assert_array_equal(bricks, dense)


# ------------------------------------------------------------- 3. env hook
def test_env_hook(monkeypatch):
    monkeypatch.delenv("HIPPT_SPARSE_GRID", raising=False)
    dense, r0 = render_cpu(smoke_box(width=32, height=24, n_grid=24))
    assert r0.info()["media"][0]["layout"] == "dense"
    monkeypatch.setenv("HIPPT_SPARSE_GRID", "1")
    hooked, r1 = render_cpu(smoke_box(width=32, height=24, n_grid=24))
    mi = r1.info()["media"][0]
    assert mi["layout"] == "bricks" and mi["n_bricks"] > 0
    np.testing.assert_array_equal(hooked, dense)
    # read per Scene, not cached
    monkeypatch.setenv("HIPPT_SPARSE_GRID", "0")
    _, r2 = render_cpu(smoke_box(width=32, height=24, n_grid=24), spp=1)
    assert r2.info()["media"][0]["layout"] == "dense"


# ----------------------------------------------------------- 4. hot reload
def test_hot_reload_scale():
    imgs = []
    for sparse in (False, True):
        d = smoke_box(width=32, height=24, n_grid=24)
        if sparse:
            sparsified(d)
        r = hippt.PythonRenderer(d, device_id=-1)
        before = r.render(spp=2).numpy().copy()
        r.scene.set_medium(0, scale=0.25)
        r.renderer.reset()
        after = r.render(spp=2).numpy().copy()
        assert not np.array_equal(before, after)
        imgs.append(after)
    np.testing.assert_array_equal(imgs[1], imgs[0])


# ----------------------------------------------------------- 5. empty grid
def test_empty_grid_is_vacuum():
    zero = np.zeros((17, 40, 24), np.float32)
    dense, _ = render_cpu(hand_built(zero))
    empty = SparseGrid((17, 40, 24), np.zeros((0, 3), np.int32),
                       np.zeros((0, 8, 8, 8), np.float32))
    bricks, r = render_cpu(hand_built(empty))
    mi = r.info()["media"][0]
    assert mi["layout"] == "bricks" and mi["n_bricks"] == 0
    np.testing.assert_array_equal(bricks, dense)
    # with an (empty) temperature pool too
    both, _ = render_cpu(hand_built(empty, SparseGrid.from_dense(zero)))
    np.testing.assert_array_equal(both, dense)
    # the container is in view: a non-empty grid changes the image
    smoky, _ = render_cpu(hand_built(SparseGrid.from_dense(random_brick_grid((17, 40, 24)))))
    assert not np.array_equal(smoky, dense)


# ------------------------------------------------- 6. NanoVDB sparse read
@pytest.mark.parametrize("codec", ["none", "zip"])
def test_nvdb_sparse_read_matches_dense(codec, tmp_path):
    a = random_brick_grid((56, 24, 40), seed=21)
    p = str(tmp_path / "g.nvdb")
    # origin not a multiple of 8: the writer's leaves sit at unaligned index
    # origins, the sparse reader anchors bricks at index_min
    write_nvdb(p, a, voxel_size=0.25, origin=(3, 5, 6), codec=codec)
    gd = read_nvdb(p)[0]
    gs = read_nvdb(p, sparse=True)[0]
    assert "dense" not in gs and "sparse" not in gd
    np.testing.assert_array_equal(gd["dense"], a)
    np.testing.assert_array_equal(gs["sparse"].to_dense(), gd["dense"])
    assert gs["sparse"].n_bricks == numpy_brick_count(a)
    for k in ("name", "index_min", "voxel_size", "world_min", "world_max",
              "grid_class", "background", "version", "map_scale"):
        assert gs[k] == gd[k], k


def _shift_leaf_origins(path, out, delta):
    """Rewrite an uncompressed single-grid file so every leaf origin and the
    index bbox min move by different amounts: leaves then straddle bricks."""
    from hippt.scene.nvdb import GRID_DATA_SIZE, LEAF_SIZE
    data = bytearray(open(path, "rb").read())
    name_size, = struct.unpack_from("<I", data, 16 + 136)
    g0 = 16 + 176 + name_size
    leaf_off, _lo, _up, root_off = struct.unpack_from("<4Q", data, g0 + GRID_DATA_SIZE)
    n_leaf, = struct.unpack_from("<I", data, g0 + GRID_DATA_SIZE + 32)
    for i in range(n_leaf):
        base = g0 + GRID_DATA_SIZE + leaf_off + i * LEAF_SIZE
        org = struct.unpack_from("<3i", data, base)
        struct.pack_into("<3i", data, base, *(o + d for o, d in zip(org, delta)))
    root = g0 + GRID_DATA_SIZE + root_off
    ib = list(struct.unpack_from("<6i", data, root))
    for a in range(3):
        ib[3 + a] += delta[a]                  # bbox max grows, min stays
    struct.pack_into("<6i", data, root, *ib)
    open(out, "wb").write(bytes(data))


def test_nvdb_leaves_straddling_bricks(tmp_path):
    """Leaf origin minus index_min not a multiple of 8: each leaf lands in up
    to 8 bricks and must still equal the dense read."""
    a = random_brick_grid((24, 16, 32), empty_frac=0.4, seed=8)
    p, q = str(tmp_path / "a.nvdb"), str(tmp_path / "b.nvdb")
    write_nvdb(p, a, origin=(0, 0, 0))
    _shift_leaf_origins(p, q, (3, 5, 6))
    gd = read_nvdb(q)[0]
    gs = read_nvdb(q, sparse=True)[0]
    assert gd["dense"].shape == (24 + 6, 16 + 5, 32 + 3)
    np.testing.assert_array_equal(gd["dense"][6:, 5:, 3:], a)
    np.testing.assert_array_equal(gs["sparse"].to_dense(), gd["dense"])


def test_nvdb_nonzero_background_raises(tmp_path):
    from hippt.scene.nvdb import GRID_DATA_SIZE
    a = random_brick_grid((16, 16, 16), seed=3)
    p = str(tmp_path / "bg.nvdb")
    write_nvdb(p, a)
    data = bytearray(open(p, "rb").read())
    name_size, = struct.unpack_from("<I", data, 16 + 136)
    g0 = 16 + 176 + name_size
    root_off, = struct.unpack_from("<Q", data, g0 + GRID_DATA_SIZE + 24)
    struct.pack_into("<f", data, g0 + GRID_DATA_SIZE + root_off + 28, 0.75)
    open(p, "wb").write(bytes(data))
    assert read_nvdb(p)[0]["background"] == 0.75
    with pytest.raises(NvdbError, match="0.75"):
        read_nvdb(p, sparse=True)


# sha256 of the file the PARENT commit's write_nvdb (dense-only writer, before
# the leaf-collection refactor) produced for _writer_fixture() with the
# arguments below; recorded by running that commit's writer once.
PARENT_WRITER_SHA256 = "35e21e51120f7734a7ba879abd10448059750e3d3d665c131cfa7eaaa47f92b5"
PARENT_WRITER_SIZE = 363176


def _writer_fixture():
    rng = np.random.default_rng(1234)
    a = rng.random((20, 33, 17)).astype(np.float32)
    a[a < 0.6] = 0
    a[:, 8:24, :] = 0
    return a


def test_write_nvdb_dense_is_byte_identical_to_parent(tmp_path):
    p = str(tmp_path / "a.nvdb")
    write_nvdb(p, _writer_fixture(), voxel_size=0.5, origin=(3, 5, 6),
               world_origin=(1.0, 2.0, 3.0))
    data = open(p, "rb").read()
    assert len(data) == PARENT_WRITER_SIZE
    assert hashlib.sha256(data).hexdigest() == PARENT_WRITER_SHA256


@pytest.mark.parametrize("shape", [(20, 33, 17), (16, 16, 16)])
def test_write_nvdb_sparse_input_equals_dense_input(shape, tmp_path):
    """Both inputs feed the same node emission: identical bytes."""
    a = _writer_fixture() if shape == (20, 33, 17) else \
        np.random.default_rng(4).random(shape).astype(np.float32) + 0.25
    p, q = str(tmp_path / "d.nvdb"), str(tmp_path / "s.nvdb")
    write_nvdb(p, a, voxel_size=0.5, origin=(3, 5, 6))
    write_nvdb(q, SparseGrid.from_dense(a), voxel_size=0.5, origin=(3, 5, 6))
    assert open(p, "rb").read() == open(q, "rb").read()


# ------------------------------------------------- 7. no dense expansion
BIG = (1024, 1024, 1024)


def big_sparse_grid():
    """40 occupied bricks scattered through a 1024^3 grid."""
    rng = np.random.default_rng(7)
    keys = rng.choice(128 ** 3, size=40, replace=False)
    coords = np.stack([keys // (128 * 128), (keys // 128) % 128, keys % 128], axis=1)
    # a cluster in the middle of the medium so the render sees some of them
    coords[:12] = [(60 + i % 2, 60 + (i // 2) % 3, 62 + i // 6) for i in range(12)]
    values = rng.random((40, 8, 8, 8)).astype(np.float32) + 0.01
    return SparseGrid(BIG, coords, values)


@pytest.fixture(scope="module")
def big_nvdb(tmp_path_factory):
    """The 1024^3 / 40-brick grid as a file (zip codec: the format's fixed
    264 KiB upper node is almost all zeros).  Shared, never modified."""
    g = big_sparse_grid()
    p = str(tmp_path_factory.mktemp("big") / "big.nvdb")
    write_nvdb(p, g, voxel_size=1.0 / 1024, codec="zip")
    return p, g


def test_no_dense_expansion(big_nvdb):
    p, g = big_nvdb
    assert g.n_bricks == 40 and g.dense_nbytes == 4 * 1024 ** 3
    assert os.path.getsize(p) < 256 * 1024
    tracemalloc.start()
    try:
        got = read_nvdb(p, sparse=True)[0]
        _cur, peak = tracemalloc.get_traced_memory()
    finally:
        tracemalloc.stop()
    assert peak < 64 << 20, peak
    s = got["sparse"]
    assert s.shape == BIG
    np.testing.assert_array_equal(s.coords, g.coords)
    np.testing.assert_array_equal(s.values, g.values)

    d = hand_built(s, width=16, height=12)
    img, r = render_cpu(d, spp=1)
    assert np.isfinite(img).all()
    mi = r.info()["media"][0]
    assert mi["layout"] == "bricks" and mi["shape"] == BIG and mi["n_bricks"] == 40
    assert mi["bytes_dense_equiv"] == 4 * 1024 ** 3
    assert mi["bytes_device"] == 0
    table_cells, super_cells, pools = 128 ** 3, 64 ** 3, 1
    expect = 4 * (table_cells + super_cells) + 2048 * 40 * pools
    assert abs(mi["bytes_host"] - expect) <= 4096, (mi["bytes_host"], expect)
    assert mi["bytes_host"] < 0.01 * mi["bytes_dense_equiv"]
    assert mi["occupancy"] == pytest.approx(40 / 128 ** 3)


# -------------------------------------------------------------- 8. grammar
XML = """<scene version="1.2">
    <medium type="grid" id="smoke">
        <rgb name="albedo" value="0.7, 0.7, 0.7"/>
        <string name="density" value="{path}"/>
        {sparse}
    </medium>
</scene>
"""


def layout_of(tmp_path, grid_file, sparse_prop):
    xml = tmp_path / "scene.xml"
    xml.write_text(XML.format(path=grid_file, sparse=sparse_prop))
    parsed = parse_xml(str(xml))
    d = smoke_box(width=16, height=12, n_grid=8)
    m = parsed.media[0]
    m.grid_lo, m.grid_hi = d.media[0].grid_lo, d.media[0].grid_hi
    d.media = [m]
    return Scene(d).info()["media"][0]["layout"], parsed.media[0].density


@pytest.mark.parametrize("prop,layout", [
    ('<string name="sparse" value="true"/>', "bricks"),
    ('<bool name="sparse" value="true"/>', "bricks"),
    ('<string name="sparse" value="false"/>', "dense"),
    ('<string name="sparse" value="auto"/>', "dense"),
    ("", "dense"),
])
def test_grammar_small_nvdb(prop, layout, tmp_path):
    a = random_brick_grid((16, 24, 16), seed=9)
    write_nvdb(str(tmp_path / "small.nvdb"), a)
    got, dens = layout_of(tmp_path, "small.nvdb", prop)
    assert got == layout
    assert isinstance(dens, SparseGrid) == (layout == "bricks")
    dense = dens.to_dense() if isinstance(dens, SparseGrid) else dens
    np.testing.assert_array_equal(dense, a)


def test_grammar_npy_forced_sparse(tmp_path):
    a = random_brick_grid((16, 24, 16), seed=10)
    np.save(str(tmp_path / "g.npy"), a)
    assert layout_of(tmp_path, "g.npy", '<string name="sparse" value="true"/>')[0] == "bricks"
    assert layout_of(tmp_path, "g.npy", "")[0] == "dense"


def test_grammar_bad_value(tmp_path):
    np.save(str(tmp_path / "g.npy"), np.ones((8, 8, 8), np.float32))
    with pytest.raises(ValueError, match="sparse"):
        layout_of(tmp_path, "g.npy", '<string name="sparse" value="maybe"/>')


def test_grammar_auto_picks_bricks_for_big_bbox(big_nvdb, tmp_path):
    p, g = big_nvdb
    layout, dens = layout_of(tmp_path, p, "")
    assert layout == "bricks" and isinstance(dens, SparseGrid) and dens.n_bricks == 40


def test_grammar_auto_nonzero_background_falls_back_dense(tmp_path, monkeypatch):
    """Under auto a nonzero-background file loads dense, with a warning (the
    threshold is lowered so a small file exercises the branch)."""
    from hippt.scene import xml_parser
    from hippt.scene.nvdb import GRID_DATA_SIZE
    a = random_brick_grid((16, 16, 16), seed=3)
    p = str(tmp_path / "bg.nvdb")
    write_nvdb(p, a)
    data = bytearray(open(p, "rb").read())
    name_size, = struct.unpack_from("<I", data, 16 + 136)
    g0 = 16 + 176 + name_size
    root_off, = struct.unpack_from("<Q", data, g0 + GRID_DATA_SIZE + 24)
    struct.pack_into("<f", data, g0 + GRID_DATA_SIZE + root_off + 28, 0.5)
    open(p, "wb").write(bytes(data))
    monkeypatch.setattr(xml_parser, "SPARSE_AUTO_BYTES", 1024)
    with pytest.warns(UserWarning, match="background"):
        layout, dens = layout_of(tmp_path, "bg.nvdb", "")
    assert layout == "dense" and isinstance(dens, np.ndarray)
    with pytest.raises(NvdbError):
        layout_of(tmp_path, "bg.nvdb", '<string name="sparse" value="true"/>')


# --------------------------------------------------------------- 9. layout
def test_medium_params_layout():
    assert C.struct_sizes()["MediumParams"] % 16 == 0


def test_info_media_lists_every_medium():
    d = smoke_box(width=16, height=12, n_grid=8)
    d.media.append(MediumDesc(type="homogeneous"))
    info = Scene(d).info()
    assert [m["layout"] for m in info["media"]] == ["dense", "homogeneous"]
    assert info["n_media"] == 2
    for m in info["media"]:
        assert set(m) == {"layout", "shape", "n_bricks", "occupancy", "bytes_host",
                          "bytes_device", "bytes_dense_equiv"}


def test_sparse_smoke_box_is_sparse():
    from hippt.scene.procedural import sparse_smoke_box
    d = sparse_smoke_box(width=16, height=12, n_grid=128)
    g = d.media[0].density
    assert isinstance(g, SparseGrid) and g.shape == (128, 128, 128)
    assert 0 < g.occupancy < 0.1
    img, r = render_cpu(d, spp=1)
    assert np.isfinite(img).all() and img[..., :3].mean() > 0
    assert r.info()["media"][0]["layout"] == "bricks"

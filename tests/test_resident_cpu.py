"""Host half of the device-resident training set (datasets.ResidentPools / GpuResidentLoader, ops.check_sel, --resident):
memory arithmetic, the rows the loader hands to the kernel against the oracle's restatement of the reference's draws,
preload validation on tiny files, the flags and the C ABI's additions.  No GPU: the kernel call is replaced by a stub."""
import argparse

import numpy as np
import pytest

from oracle import kitti_augment as K

KITTI_SHAPES = [(128, 416, 1), (128, 416, 3), (128, 416, 1)]


def test_resident_bytes_hand_arithmetic():
    from gdn_amd.datasets import resident_bytes
    assert resident_bytes(1, KITTI_SHAPES) == 128 * 416 * 5 == 266240
    assert resident_bytes(23000, KITTI_SHAPES) == 6123520000               # the ~23k-sample Eigen training set: ~6 GB
    assert resident_bytes(13444, [(128, 416, 3)]) > 2 ** 31 > resident_bytes(13443, [(128, 416, 3)])
    assert resident_bytes(26887, [(128, 416, 3)]) > 2 ** 32 > resident_bytes(26886, [(128, 416, 3)])
    assert 26888 * 128 * 416 * 3 > 2 ** 32 and 13444 * 128 * 416 * 3 > 2 ** 31      # offsets of samples a 32-bit index would wrap
    # NYU: uint16 depth + uint8 colour at 480 x 640
    assert resident_bytes(1, [(480, 640), (480, 640, 3)], [2, 1]) == 480 * 640 * 5 == 1536000
    assert resident_bytes(50000, [(480, 640), (480, 640, 3)], [2, 1]) == 76800000000
    assert resident_bytes(0, KITTI_SHAPES) == 0


def test_over_budget_is_refused_before_allocating(monkeypatch):
    import torch
    from gdn_amd import datasets as DS
    from gdn_amd._lib import GdnError
    ds = DS.SyntheticRawKitti(6, 16, 24)
    need = DS.resident_bytes(6, [(16, 24, 1), (16, 24, 3), (16, 24, 1)])
    allocated = []
    real_empty = torch.empty
    monkeypatch.setattr(DS.torch, "empty", lambda *a, **k: allocated.append(a) or real_empty(*a, **k))
    with pytest.raises(GdnError, match="needs .* GB .* budget is"):
        DS.ResidentPools(ds, "cpu", max_bytes=need - 1)
    assert not allocated
    pools = DS.ResidentPools(ds, "cpu", max_bytes=need)
    assert pools.nbytes == need and pools.n == 6 and pools.size == (16, 24)
    assert [tuple(t.shape) for t in pools.tensors] == [(6, 16, 24, 1), (6, 16, 24, 3), (6, 16, 24, 1)]
    for i in range(6):
        for j in range(3):
            assert np.array_equal(pools.tensors[j][i].numpy(), ds[i][j])


def test_preload_threads_are_bounded(monkeypatch):
    import os
    from gdn_amd import datasets as DS
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(200)))
    monkeypatch.setattr(os, "cpu_count", lambda: 1000)
    assert DS.preload_threads(0) == 16 and DS.preload_threads(64) == 16 and DS.preload_threads(3) == 3
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(5)))
    assert DS.preload_threads(0) == 5 and DS.preload_threads(16) == 5


def test_staging_buffer_is_bounded_and_chunks_cover_the_set(monkeypatch):
    """A staging buffer smaller than the set: several chunks, the last one partial, every sample in its place."""
    from gdn_amd import datasets as DS
    ds = DS.SyntheticRawKitti(11, 8, 12, seed=3)
    assert DS.STAGING_BYTES == 64 << 20
    monkeypatch.setattr(DS, "STAGING_BYTES", 4 * 8 * 12 * 5 + 7)            # 4 samples per chunk: 4 + 4 + 3
    pools = DS.ResidentPools(ds, "cpu", max_bytes=1 << 20, workers=2)
    for i in range(11):
        for j in range(3):
            assert np.array_equal(pools.tensors[j][i].numpy(), ds[i][j])


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("drop_last", [True, False])
def test_loader_rows_match_oracle_draws(monkeypatch, world, drop_last):
    """The rows GpuResidentLoader hands to the kernel over two epochs: indices from GpuAugmentLoader._epoch_order of a
    loader built with the same arguments, draws from the ORACLE's draw_params on make_rngs(seed)."""
    from gdn_amd import datasets as DS
    from gdn_amd import ops
    H, W, n, bs, seed = 16, 24, 23, 4, 9

    class Once(DS.SyntheticRawKitti):
        pass

    ds = Once(n, H, W, seed=1)
    pools = DS.ResidentPools(ds, "cpu", max_bytes=1 << 20)
    monkeypatch.setattr(Once, "__getitem__", lambda self, i: pytest.fail("dataset indexed after the preload"), raising=False)
    seen = []

    def stub(tensors, sel, train):
        assert tensors is pools.tensors and train
        seen.append(np.array(sel.numpy()))
        return tuple(sel for _ in range(3))

    monkeypatch.setattr(ops, "kitti_augment_resident", stub)
    for rank in range(world):
        kw = dict(train=True, seed=seed + rank, drop_last=drop_last, rank=rank, world=world, order_seed=seed + 1)
        loader = DS.GpuResidentLoader(ds, bs, "cpu", pools=pools, **kw)
        parent = DS.GpuAugmentLoader(ds, bs, "cpu", **kw)
        py, npr = K.make_rngs(seed + rank)
        shard = n // world if world > 1 else n
        assert len(loader) == len(parent) == (shard // bs if drop_last else -(-shard // bs))
        for epoch in range(2):
            order = parent._epoch_order()
            del seen[:]
            batches = list(loader)
            assert len(batches) == len(seen) == len(loader)
            for b, rows in enumerate(seen):
                idxs = order[b * bs:(b + 1) * bs]
                want = [(i,) + K.draw_params(H, W, py, npr) for i in idxs]
                assert rows.dtype == np.int32 and rows.tolist() == [list(w) for w in want]
                if b == len(seen) - 1:
                    assert loader.last_params == [w[1:] for w in want]


def test_validation_rows_carry_the_index_only(monkeypatch):
    from gdn_amd import datasets as DS
    from gdn_amd import ops
    ds = DS.SyntheticRawKitti(5, 8, 12)
    seen = []
    monkeypatch.setattr(ops, "kitti_augment_resident", lambda t, sel, train: seen.append((sel.numpy().tolist(), train)) or (sel,) * 3)
    loader = DS.GpuResidentLoader(ds, 2, "cpu", train=False, max_bytes=1 << 20)
    list(loader)
    assert seen == [([[0, 0, 8, 12, 0, 0], [1, 0, 8, 12, 0, 0]], False), ([[2, 0, 8, 12, 0, 0], [3, 0, 8, 12, 0, 0]], False),
                    ([[4, 0, 8, 12, 0, 0]], False)]


def test_check_sel_refuses_rows_the_device_would_not():
    from gdn_amd import ops
    from gdn_amd._lib import GdnError
    ok = [[3, 1, 18, 26, 2, 1], [0, 0, 16, 24, 0, 0]]
    assert ops.check_sel(ok, 4, 16, 24).dtype == np.int32
    for bad in ([[4, 0, 16, 24, 0, 0]], [[-1, 0, 16, 24, 0, 0]], [[0, 2, 16, 24, 0, 0]], [[0, 0, 15, 24, 0, 0]],
                [[0, 0, 16, 24, 0, 1]], [[0, 0, 18, 24, 3, 0]], [[0, 0, 16, 30, 0, -1]]):
        with pytest.raises(GdnError):
            ops.check_sel(bad, 4, 16, 24)
    assert ops.check_sel([[3, 9, 9, 9, 9, 9]], 4, 16, 24, train=False).shape == (1, 6)      # validation: the index only
    with pytest.raises(GdnError):
        ops.check_sel([[4, 0, 16, 24, 0, 0]], 4, 16, 24, train=False)
    with pytest.raises(GdnError):
        ops.check_sel(np.zeros((0, 6)), 4, 16, 24)


def _write_scene(root, scene, n, size=(16, 24), seed=0):
    from PIL import Image
    r = np.random.RandomState(seed)
    (root / scene / "color_gt2").mkdir(parents=True)
    (root / scene / "gt").mkdir()
    for i in range(n):
        Image.fromarray(r.randint(0, 256, size + (3,)).astype(np.uint8)).save(root / scene / ("%07d.jpg" % i))
        Image.fromarray(r.randint(0, 256, size).astype(np.uint8)).save(root / scene / "color_gt2" / ("%07d.png" % i))
        Image.fromarray(r.randint(0, 256, size).astype(np.uint8)).save(root / scene / "gt" / ("%07d.png" % i))


def test_preload_reads_the_reference_layout(tmp_path):
    from gdn_amd import datasets as DS
    _write_scene(tmp_path, "s1", 3, seed=1)
    _write_scene(tmp_path, "s2", 3, seed=2)
    (tmp_path / "train.txt").write_text("s1\ns2\n")
    ds = DS.SequenceFolder(tmp_path, argparse.Namespace(img_test=False), seed=1, train=True)
    pools = DS.ResidentPools(ds, "cpu", max_bytes=1 << 20)
    assert pools.n == 6 and pools.size == (16, 24) and pools.kind == "kitti"
    for i in range(6):
        for j in range(3):
            assert np.array_equal(pools.tensors[j][i].numpy(), ds[i][j])


def test_mixed_size_scene_is_refused_naming_the_file(tmp_path):
    from PIL import Image
    from gdn_amd import datasets as DS
    from gdn_amd._lib import GdnError
    _write_scene(tmp_path, "s1", 4, seed=1)
    odd = tmp_path / "s1" / "color_gt2" / "0000002.png"
    Image.fromarray(np.zeros((16, 26), np.uint8)).save(odd)
    (tmp_path / "train.txt").write_text("s1\n")
    ds = DS.SequenceFolder(tmp_path, argparse.Namespace(img_test=False), seed=1, train=True)
    with pytest.raises(GdnError) as e:
        DS.ResidentPools(ds, "cpu", max_bytes=1 << 20)
    assert str(odd) in str(e.value) and "(16, 26, 1)" in str(e.value)


def test_sixteen_bit_png_is_refused_naming_the_file(tmp_path):
    from PIL import Image
    from gdn_amd import datasets as DS
    from gdn_amd._lib import GdnError
    _write_scene(tmp_path, "s1", 4, seed=1)
    deep = tmp_path / "s1" / "gt" / "0000001.png"
    Image.fromarray((np.arange(16 * 24).reshape(16, 24) * 100).astype(np.uint16)).save(deep)
    (tmp_path / "train.txt").write_text("s1\n")
    ds = DS.SequenceFolder(tmp_path, argparse.Namespace(img_test=False), seed=1, train=True)
    assert any(ds[i][2].dtype == np.float32 for i in range(4))          # what the non-resident loader bytescales
    with pytest.raises(GdnError) as e:
        DS.ResidentPools(ds, "cpu", max_bytes=1 << 20)
    assert str(deep) in str(e.value) and "uint8" in str(e.value)


def test_nyu_pools_hold_uint16_depth_and_refuse_fractions(tmp_path):
    from PIL import Image
    from gdn_amd import datasets as DS
    from gdn_amd._lib import GdnError
    r = np.random.RandomState(0)
    for sub in ("train/train_depths", "train/train_colors"):
        (tmp_path / sub).mkdir(parents=True)
    for i in range(3):
        Image.fromarray(r.randint(0, 65536, (12, 20)).astype(np.uint16)).save(tmp_path / "train/train_depths" / ("%05d.png" % i))
        Image.fromarray(r.randint(0, 256, (12, 20, 3)).astype(np.uint8)).save(tmp_path / "train/train_colors" / ("%05d.png" % i))
    ds = DS.NYUdataset(str(tmp_path), None, seed=3, train=True)
    pools = DS.ResidentPools(ds, "cpu", max_bytes=1 << 20)
    assert pools.kind == "nyu" and pools.size == (12, 20) and pools.nbytes == 3 * 12 * 20 * 5
    import torch
    assert pools.tensors[0].dtype == torch.uint16 and pools.tensors[1].dtype == torch.uint8
    for i in range(3):
        assert np.array_equal(pools.tensors[0][i].numpy().astype(np.float32), ds[i][0][:, :, 0])
        assert np.array_equal(pools.tensors[1][i].numpy(), ds[i][1])

    class Fractional:
        samples = ds.samples

        def __len__(self):
            return 3

        def __getitem__(self, i):
            d, c, _ = ds[i]
            return (d + np.float32(0.5) if i == 2 else d), c, d

    with pytest.raises(GdnError, match="integral"):
        DS.ResidentPools(Fractional(), "cpu", kind="nyu", max_bytes=1 << 20)


def test_resident_flags_parse_and_synthetic_is_refused():
    from gdn_amd import GDN_main, option
    a = option.parse_args(["x", "--resident"])
    assert a.resident is True and a.resident_gb is None
    assert option.parse_args(["x"]).resident is False
    assert option.parse_args(["x", "--resident", "--resident_gb", "7.5"]).resident_gb == 7.5
    with pytest.raises(RuntimeError, match="--resident .*--synthetic"):
        GDN_main.run(option.parse_args(["x", "--resident", "--synthetic"]))
    with pytest.raises(RuntimeError, match="--resident"):
        GDN_main.run(option.parse_args(["x", "--resident", "--dataset", "NYU", "--mode", "DtoD_test"]))


def test_abi_gains_two_entry_points_at_the_same_revision():
    from gdn_amd import _lib
    assert "gdn_kitti_augment_resident" in _lib._SIGS and "gdn_gather_samples" in _lib._SIGS
    assert _lib.ABI_VERSION == 223
    assert _lib.lib.gdn_version() == 223
    # argument checks that need no device: null pools, empty batch, element widths other than 1 or 2
    with pytest.raises(_lib.GdnError, match="gdn_kitti_augment_resident"):
        _lib.lib.gdn_kitti_augment_resident(None, 1, None, 3, None, 1, 8, 8, None, 1, 1, None, None, None, None)
    with pytest.raises(_lib.GdnError, match="gdn_gather_samples"):
        _lib.lib.gdn_gather_samples(None, 1, None, 1, 8, 0, None, None)

"""The mesh-extraction route without a GPU: the properties of the fp64 oracles of tests/mesh_oracle.py themselves, the mesh `.ply`
codec, the bounding sphere, the torch-only cluster filter, and the contract of the new ops (GPU only, float32, errors that name the
argument; the command line answers --help without a GPU)."""
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mesh_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_all_256_sign_patterns():
    """Triangles per tetrahedron follow the number of inside corners; every triangle's normal points away from the inside corners."""
    origin, step = np.zeros(3, np.float32), np.ones(3, np.float32)
    for pattern in range(256):
        inside = np.array([(pattern >> m) & 1 for m in range(8)], bool)
        vol = np.where(inside, -1.0, 1.0).astype(np.float32).reshape(2, 2, 2)
        out = MO.marching_tetrahedra(vol, 0.0, origin, step)
        expected = sum({0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[sum(inside[c] for c in tet)] for tet in MO.TETS)
        assert out["counts"].tolist() == [expected] and out["keys"].shape[0] == 3 * expected
        assert (pattern in (0, 255)) == (expected == 0)
        if expected:
            tri = out["vertices"].reshape(-1, 3, 3)
            normal = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
            centre_in = MO._OFF[inside].mean(0)
            assert (np.linalg.norm(normal, axis=-1) > 0).all()
            if inside.sum() in (1, 7):          # a single corner cut off (or left): every normal points away from / towards it
                away = tri.mean(1) - (centre_in if inside.sum() == 1 else MO._OFF[~inside].mean(0))
                sign = 1 if inside.sum() == 1 else -1
                assert (np.einsum("ij,ij->i", normal, away) * sign > 0).all()
            assert np.array_equal(out["keys"] % 8 < 7, np.ones_like(out["keys"], bool)) and (out["keys"] >= 0).all()


@pytest.mark.parametrize("name, chi, analytic, measured", [("sphere 9", 2, None, None), ("sphere 17", 2, 4 / 3 * math.pi * 0.125, -0.020),
                                                           ("torus 24", 0, 2 * math.pi ** 2 * 0.5 * 0.04, -0.016)])
def test_oracle_topology(name, chi, analytic, measured):
    vol, origin, step = MO.torus_volume(24) if name == "torus 24" else MO.sphere_volume(int(name.split()[1]))
    out = MO.marching_tetrahedra(vol, 0.0, origin, step)
    v, f, keys = MO.index_soup(out["vertices"], out["keys"])
    assert MO.is_closed_oriented(f) and MO.euler(v.shape[0], f) == chi
    volume = MO.signed_volume(v, f)
    assert volume > 0
    if analytic is not None:
        assert abs(volume / analytic - 1) <= 0.03 and abs(volume / analytic - 1 - measured) < 2e-3
    # equal keys hold equal positions: the merge loses nothing
    assert np.array_equal(v[np.searchsorted(keys, out["keys"])], out["vertices"])


def test_oracle_blocks_share_keys_and_positions():
    vol, origin, step = MO.sphere_volume(17)
    whole = MO.marching_tetrahedra(vol, 0.0, origin, step)
    a = MO.marching_tetrahedra(vol[:9], 0.0, origin, step, (17, 17, 17), (0, 0, 0))
    b = MO.marching_tetrahedra(vol[8:], 0.0, origin, step, (17, 17, 17), (8, 0, 0))
    wv, wf, wk = MO.index_soup(whole["vertices"], whole["keys"])
    mv, mf, mk = MO.index_soup(np.concatenate([a["vertices"], b["vertices"]]), np.concatenate([a["keys"], b["keys"]]))
    assert np.array_equal(wk, mk) and np.array_equal(wv, mv) and len(np.intersect1d(a["keys"], b["keys"])) > 0
    order = lambda f: f[np.lexsort(f.T[::-1])]
    assert np.array_equal(order(wf), order(mf))


def test_oracle_two_calls_equal_one_and_the_torch_restatement_agrees():
    full, _, geo = MO.orbit_cameras(7, 37, 50)
    depth, rgb = MO.sphere_maps(geo, 37, 50)
    centre = (0.03, -0.02, 0.01)
    for contract in (False, True):
        pts = MO.scene_points(1500, contract, centre, 1.0, seed=2)
        args = dict(center=centre, radius=1.0, voxel_size=2 / 64, contract=contract)
        one = MO.fuse(pts, full, depth, rgb, **args)
        first = MO.fuse(pts, full[:2], depth[:2], rgb[:2], **args)
        # (the oracle keeps its state in fp64: handing it on as float32 is what the kernel's two calls do, so compare to rounding)
        two = MO.fuse(pts, full[2:], depth[2:], rgb[2:], state=(first["tsdf"], first["weight"], first["color"]), **args)
        assert np.array_equal(one["weight"], two["weight"])
        assert np.abs(one["tsdf"] - two["tsdf"]).max() < 1e-6 and np.abs(one["color"] - two["color"]).max() < 1e-6
        live = ((one["weight"] > 2) & (np.abs(one["tsdf"]) < 1)).mean()
        assert live > 0.25 and one["flagged"].mean() < 0.02
        t = lambda a: torch.from_numpy(np.asarray(a)).double()
        tsdf, weight, color = MO.fuse_torch(t(pts), t(full), t(depth), t(rgb), center=t(np.asarray(centre, np.float32)), radius=1.0,
                                            voxel_size=float(np.float32(2 / 64)), contract=contract)
        firm = ~one["flagged"]
        assert np.array_equal(weight.numpy()[firm], one["weight"][firm])
        assert np.abs(tsdf.numpy() - one["tsdf"])[firm].max() < 1e-12 and np.abs(color.numpy() - one["color"])[firm].max() < 1e-12


def test_ply_mesh_round_trip(tmp_path):
    import gspl_amd  # noqa: F401
    from gspl_amd.formats import read_ply_mesh, write_ply_mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1.5, 0], [0, 0, -2.25]], np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)
    c = np.array([[0, 0.5, 1], [1.7, -0.2, 0.25], [0.1, 0.2, 0.3], [0.999, 0.002, 0.498]])
    path = str(tmp_path / "sub" / "mesh.ply")
    write_ply_mesh(path, v, f, c)
    raw = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 4\nproperty list uchar int vertex_indices\nend_header\n")
    assert raw.startswith(header) and len(raw) == len(header) + 4 * 15 + 4 * 13
    assert raw[len(header):len(header) + 15] == np.zeros(3, "<f4").tobytes() + bytes([0, 128, 255])
    assert raw[len(header) + 60:len(header) + 73] == bytes([3]) + np.array([0, 1, 2], "<i4").tobytes()
    rv, rf, rc = read_ply_mesh(path)
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and rf.dtype == np.int32
    assert rc.tolist() == [[0, 128, 255], [255, 0, 64], [26, 51, 76], [255, 1, 127]]
    plain = str(tmp_path / "plain.ply")
    write_ply_mesh(plain, v, f)
    assert open(plain, "rb").read().startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\n"
                                               b"property float z\nelement face 4\nproperty list uchar int vertex_indices\nend_header\n")
    rv, rf, rc = read_ply_mesh(plain)
    assert np.array_equal(rv, v) and np.array_equal(rf, f) and rc is None
    write_ply_mesh(plain, np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    rv, rf, rc = read_ply_mesh(plain)
    assert rv.shape == (0, 3) and rf.shape == (0, 3)
    with pytest.raises(ValueError, match="outside"):
        write_ply_mesh(plain, v, f + 1)


def test_bounding_sphere_of_a_camera_ring():
    """Eight cameras on a ring of radius 3 around (1, 2, 0.5), all looking at that point, one of them moved in to distance 2: the
    focus point is the ring's centre and the radius the nearest camera's distance."""
    import gspl_amd  # noqa: F401
    from gspl_amd import mesh
    centre = np.array([1.0, 2.0, 0.5])
    cameras = []
    for i in range(8):
        a = 2 * math.pi * i / 8
        eye = centre + (2.0 if i == 3 else 3.0) * np.array([math.cos(a), math.sin(a), 0.0])
        fwd = (centre - eye) / np.linalg.norm(centre - eye)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        down = np.cross(fwd, right)
        w2c = np.eye(4)
        w2c[:3, :3] = np.stack([right, down, fwd])
        w2c[:3, 3] = -w2c[:3, :3] @ eye
        cameras.append(types.SimpleNamespace(world_to_camera=torch.from_numpy(w2c.T).float()))
    got_centre, radius = mesh.estimate_bounding_sphere(cameras)
    assert np.abs(got_centre - centre).max() < 1e-5 and abs(radius - 2.0) < 1e-5


def test_keep_largest_clusters_on_the_cpu():
    import gspl_amd  # noqa: F401
    from gspl_amd import mesh
    parts, offset = [], 0
    for n, shift in ((17, 0.0), (9, 5.0)):
        vol, origin, step = MO.sphere_volume(n)
        out = MO.marching_tetrahedra(vol, 0.0, origin, step)
        v, f, _ = MO.index_soup(out["vertices"] + shift, out["keys"])
        parts.append((v, f))
    blob = np.ones((3, 3, 3), np.float32)
    blob[1, 1, 1] = -1.0
    out = MO.marching_tetrahedra(blob, 0.0, np.array([20, 0, 0], np.float32), np.ones(3, np.float32))
    parts.append(MO.index_soup(out["vertices"], out["keys"])[:2])
    sizes = [p[1].shape[0] for p in parts]
    assert sizes[2] == 24 and sizes[0] > sizes[1] > 50
    offsets = np.cumsum([0] + [p[0].shape[0] for p in parts])
    v = torch.from_numpy(np.concatenate([p[0] for p in parts])).float()
    f = torch.from_numpy(np.concatenate([p[1] + o for p, o in zip(parts, offsets)]))
    labels = mesh.face_clusters(f, v.shape[0])
    assert torch.unique(labels).numel() == 3 and np.array_equal(np.sort(np.bincount(MO.components(f.numpy())[0])), np.sort(sizes))
    v1, f1 = mesh.keep_largest_clusters(v, f, cluster_to_keep=1)
    assert f1.shape[0] == sizes[0] and v1.shape[0] == parts[0][0].shape[0] and torch.equal(v1, v[:v1.shape[0]])
    v2, f2 = mesh.keep_largest_clusters(v, f)                        # fewer clusters than cluster_to_keep: min_triangles decides
    assert f2.shape[0] == sizes[0] + sizes[1] and int(f2.max()) == v2.shape[0] - 1
    v3, f3 = mesh.keep_largest_clusters(v, f, cluster_to_keep=2, min_triangles=1)
    assert f3.shape[0] == sizes[0] + sizes[1]
    empty = mesh.keep_largest_clusters(v, f[:0])
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


def test_ops_refuse_cpu_tensors_and_other_dtypes():
    import gspl_amd  # noqa: F401
    from gspl_amd import ops
    state = (torch.ones(4), torch.ones(4), None)
    table, views, depth, pts = torch.zeros(16), torch.zeros(2, 4, 4), torch.zeros(2, 3, 3), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match=r"tsdf: the mesh ops run on the GPU only"):
        ops.tsdf_fuse(state, table, views, depth, points=pts)
    with pytest.raises(RuntimeError, match=r"volume: the mesh ops run on the GPU only"):
        ops.marching_tetrahedra(torch.zeros(3, 3, 3), 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError, match=r"device: the mesh ops run on the GPU only"):
        ops.tsdf_init(4, True, "cpu")
    with pytest.raises(RuntimeError, match=r"device: the mesh ops run on the GPU only"):
        ops.tsdf_table(device="cpu")
    # dtype and shape checks come before anything touches a device: a tensor subclass that claims to be on the GPU stands in for one
    class OnGpu(torch.Tensor):
        is_cuda = True
    gpu = lambda t: t.as_subclass(OnGpu)
    with pytest.raises(RuntimeError, match=r"volume: float32 is needed, got torch.float64"):
        ops.marching_tetrahedra(gpu(torch.zeros(3, 3, 3, dtype=torch.float64)), 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError, match=r"weight: float32 is needed, got torch.float16"):
        ops.tsdf_fuse((gpu(torch.ones(4)), gpu(torch.ones(4).half()), None), gpu(table), gpu(views), gpu(depth), points=gpu(pts))
    with pytest.raises(RuntimeError, match=r"depth: float32 is needed, got torch.float64"):
        ops.tsdf_fuse((gpu(torch.ones(4)), gpu(torch.ones(4)), None), gpu(table), gpu(views), gpu(depth.double()), points=gpu(pts))
    with pytest.raises(ValueError, match=r"points must be \[4, 3\]"):
        ops.tsdf_fuse((gpu(torch.ones(4)), gpu(torch.ones(4)), None), gpu(table), gpu(views), gpu(depth), points=gpu(torch.zeros(5, 3)))
    with pytest.raises(ValueError, match=r"needs `points` or `lattice`"):
        ops.tsdf_fuse((gpu(torch.ones(4)), gpu(torch.ones(4)), None), gpu(table), gpu(views), gpu(depth))
    with pytest.raises(ValueError, match=r"does not describe the state's 4 samples"):
        ops.tsdf_fuse((gpu(torch.ones(4)), gpu(torch.ones(4)), None), gpu(table), gpu(views), gpu(depth), lattice=(2, 2, 2))
    with pytest.raises(ValueError, match=r"volume must be \[X, Y, Z\]"):
        ops.marching_tetrahedra(gpu(torch.zeros(3, 3)), 0.0, (0, 0, 0), (1, 1, 1))


def test_new_entry_points_are_in_the_header_and_the_library():
    import ctypes
    import gspl_amd  # noqa: F401
    from gspl_amd import _lib
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("gspl_tsdf_fuse", "gspl_mtet_count", "gspl_mtet_emit"):
        assert name in _lib.exported_symbols() and hasattr(handle, name)
    P, I, Q = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _lib._SIGNATURES["gspl_tsdf_fuse"] == (I, [Q, P] + [I] * 9 + [P, I, I, I, P, P, P, P, P, P, P])
    assert _lib._SIGNATURES["gspl_mtet_emit"] == (I, [I, I, I, P, ctypes.c_float, P] + [I] * 6 + [P, Q, P, P, P])
    assert _lib.GSPL_TSDF_TABLE_FLOATS == 16 and _lib.GSPL_ABI_VERSION == 39
    lib = _lib.lib()
    # argument checks happen before any launch: refused without a GPU
    assert lib.gspl_tsdf_fuse(-1, None, 0, 0, 0, 0, 0, 0, 0, 0, 0, None, 1, 1, 1, None, None, None, None, None, None, None) != 0
    assert b"tsdf_fuse" in lib.gspl_last_error()
    assert lib.gspl_tsdf_fuse(8, None, 2, 2, 2, 0, 0, 0, 2, 2, 2, None, 1, 1, 1, None, None, None, None, None, None, None) != 0      # NULL table
    assert lib.gspl_mtet_emit(3, 3, 3, None, 0.0, None, 3, 3, 2, 0, 0, 0, None, 5, None, None, None) != 0                                # block leaves G
    assert lib.gspl_mtet_count(1, 5, 5, None, 0.0, None, None) == 0 and lib.gspl_mtet_emit(5, 5, 1, None, 0.0, None, 5, 5, 1, 0, 0, 0, None, 0, None, None, None) == 0


def test_command_line_help_needs_no_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "gspl_amd.mesh", "--help"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    for flag in ("model_path", "--dataset_path", "--voxel_size", "--depth_trunc", "--sdf_trunc", "--num_cluster", "--unbounded", "--mesh_res"):
        assert flag in res.stdout
    import gspl_amd  # noqa: F401
    from gspl_amd import mesh
    args = mesh.parser().parse_args(["some/model"])
    assert (args.dataset_path, args.voxel_size, args.depth_trunc, args.sdf_trunc, args.num_cluster, args.unbounded, args.mesh_res) == \
        (None, -1.0, -1.0, -1.0, 50, False, 1024)

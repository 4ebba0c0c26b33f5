"""PLY scene I/O (include/gsr_ply.h, csrc/ply.cpp, gaussian_splatting_amd/ply.py).

The reference writes and reads its scenes with `plyfile` (scene/gaussian_model.py:288-376,
scene/dataset_readers.py:120-143), which this image lacks, and its tests hold no PLY file:
no reference fixture exists.  Pinned here by the PLY 1.0 format itself (header
bytes as plyfile emits them: "ply", "format binary_little_endian 1.0", "element vertex N",
"property float <name>" / "property uchar <name>", "end_header"), by hand-built files in the
other encodings the reader must accept (ascii with comments, big-endian with mixed types,
an element with a list property before "vertex"), and by the reference's attribute order and
SH layout.  The reference's own storePly / fetchPly / save_ply / construct_list_of_attributes,
compiled from its source with the drop-in ``plyfile`` package of this repository, wrote the
files recorded under tests/golden/ (make_golden.py): ours must be byte-identical to them,
read back identical arrays, and the drop-in must rewrite them unchanged.  The reader/writer is host code, so these run on the CPU except the load_ply test,
which creates the parameters on the GPU as the reference does.
"""
import os
import struct

import numpy as np
import pytest
import torch

from gaussian_splatting_amd import ply


def test_header_bytes_and_roundtrip(tmp_path):
    p = str(tmp_path / "a.ply")
    rng = np.random.default_rng(0)
    a = rng.standard_normal((5, 2)).astype(np.float32)
    b = np.array([0, 1, 127, 200, 255], np.uint8)
    ply.write_vertex(p, [("x", a[:, 0]), ("y", a[:, 1]), ("red", b)])  # strided float columns
    raw = open(p, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\n"
              b"property uchar red\nend_header\n")
    assert raw.startswith(header)
    body = raw[len(header):]
    assert len(body) == 5 * 9
    for i in range(5):
        x, y, r = struct.unpack_from("<ffB", body, 9 * i)
        assert (x, y, r) == (a[i, 0], a[i, 1], b[i])
    n, names = ply.vertex_properties(p)
    assert n == 5 and names == ["x", "y", "red"]
    c = ply.read_vertex(p, ["red", "x"])
    np.testing.assert_array_equal(c["x"], a[:, 0])
    np.testing.assert_array_equal(c["red"], b.astype(np.float32))


def test_reads_ascii_with_comments(tmp_path):
    p = str(tmp_path / "ascii.ply")
    with open(p, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment made by hand\nobj_info test\nelement vertex 3\n"
                "property float x\nproperty double y\nproperty uchar red\nend_header\n"
                "1.5 -2.25 7\n0 1e-3 255\n-3 4 0\n")
    c = ply.read_vertex(p, ["x", "y", "red"])
    np.testing.assert_array_equal(c["x"], np.float32([1.5, 0, -3]))
    np.testing.assert_array_equal(c["y"], np.float32([-2.25, 1e-3, 4]))
    np.testing.assert_array_equal(c["red"], np.float32([7, 255, 0]))


def test_reads_big_endian_mixed_types_and_list_element_first(tmp_path):
    p = str(tmp_path / "be.ply")
    hdr = ("ply\nformat binary_big_endian 1.0\nelement face 2\nproperty list uchar int vertex_indices\n"
           "element vertex 2\nproperty short a\nproperty float x\nproperty double d\nproperty uint u\n"
           "property list uchar float extra\nend_header\n").encode()
    body = struct.pack(">BiiiBii", 3, 0, 1, 2, 2, 5, 6)  # two faces
    body += struct.pack(">hfdIBff", -7, 1.25, 3.5, 4000000000, 2, 9.0, 8.0)
    body += struct.pack(">hfdIB", 12, -0.5, -1e10, 1, 0)
    open(p, "wb").write(hdr + body)
    n, names = ply.vertex_properties(p)
    assert n == 2 and names == ["a", "x", "d", "u", "extra"]
    c = ply.read_vertex(p, ["a", "x", "d", "u"])
    np.testing.assert_array_equal(c["a"], np.float32([-7, 12]))
    np.testing.assert_array_equal(c["x"], np.float32([1.25, -0.5]))
    np.testing.assert_array_equal(c["d"], np.float32([3.5, -1e10]))
    np.testing.assert_array_equal(c["u"], np.float32([4000000000, 1]))


def test_errors(tmp_path):
    from gaussian_splatting_amd._lib import GsrError

    p = str(tmp_path / "bad.ply")
    open(p, "w").write("not a ply\n")
    with pytest.raises(GsrError, match="not a PLY"):
        ply.vertex_properties(p)
    q = str(tmp_path / "ok.ply")
    ply.write_vertex(q, [("x", np.zeros(3, np.float32))])
    with pytest.raises(GsrError, match="no vertex property 'y'"):
        ply.read_vertex(q, ["y"])
    with open(q, "r+b") as f:  # truncate the body
        f.truncate(os.path.getsize(q) - 2)
    with pytest.raises(GsrError, match="truncated"):
        ply.read_vertex(q, ["x"])


class _CpuModel:
    def __init__(self, P, sh_degree, rng):
        K = (sh_degree + 1) ** 2
        self.max_sh_degree = sh_degree
        self._xyz = torch.tensor(rng.standard_normal((P, 3)), dtype=torch.float32)
        self._features_dc = torch.tensor(rng.standard_normal((P, 1, 3)), dtype=torch.float32)
        self._features_rest = torch.tensor(rng.standard_normal((P, K - 1, 3)), dtype=torch.float32)
        self._opacity = torch.tensor(rng.standard_normal((P, 1)), dtype=torch.float32)
        self._scaling = torch.tensor(rng.standard_normal((P, 3)), dtype=torch.float32)
        self._rotation = torch.tensor(rng.standard_normal((P, 4)), dtype=torch.float32)


def test_save_ply_layout(tmp_path):
    """Property names and order of construct_list_of_attributes (gaussian_model.py:288-300) and
    the channel-major SH flattening of save_ply (:306-307)."""
    m = _CpuModel(37, 3, np.random.default_rng(1))
    p = str(tmp_path / "pc" / "point_cloud.ply")
    ply.save_ply(m, p)
    n, names = ply.vertex_properties(p)
    expect = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(45)]
              + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
    assert n == 37 and names == expect
    c = ply.read_vertex(p, names)
    rest = m._features_rest.numpy()
    for ch in range(3):
        for k in range(15):
            np.testing.assert_array_equal(c[f"f_rest_{ch * 15 + k}"], rest[:, k, ch])
        np.testing.assert_array_equal(c[f"f_dc_{ch}"], m._features_dc.numpy()[:, 0, ch])
    assert not c["nx"].any()
    np.testing.assert_array_equal(c["rot_3"], m._rotation.numpy()[:, 3])


def test_store_fetch_ply(tmp_path):
    p = str(tmp_path / "points3D.ply")
    rng = np.random.default_rng(2)
    xyz = rng.standard_normal((100, 3))
    rgb = rng.integers(0, 256, (100, 3)).astype(np.uint8)
    ply.store_ply(p, xyz, rgb)
    pc = ply.fetch_ply(p)
    np.testing.assert_array_equal(pc.points, xyz.astype(np.float32))
    np.testing.assert_array_equal(pc.colors, rgb / 255.0)
    assert pc.normals.shape == (100, 3) and not pc.normals.any()


@pytest.mark.gpu
def test_load_ply_roundtrip(tmp_path):
    src = _CpuModel(1001, 3, np.random.default_rng(3))
    p = str(tmp_path / "point_cloud.ply")
    ply.save_ply(src, p)
    dst = type("M", (), {"max_sh_degree": 3})()
    ply.load_ply(dst, p)
    for a in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        got = getattr(dst, a)
        assert got.is_cuda and got.requires_grad and got.is_contiguous()
        assert torch.equal(got.detach().cpu(), getattr(src, a)), a
    assert dst.active_sh_degree == 3


# ---- the reference's own PLY code, run through the drop-in plyfile, recorded in tests/golden/ ----
# tests/golden/make_golden.py ran the reference's storePly / fetchPly / save_ply /
# construct_list_of_attributes (with this repository's plyfile in their globals) on the inputs below and
# stored the files they wrote and what they read back; the inputs are rebuilt here from their seeds.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def reference_store_inputs():
    rng = np.random.default_rng(4)
    xyz = rng.standard_normal((500, 3))
    rgb = rng.integers(0, 256, (500, 3)).astype(np.uint8)
    return xyz, rgb


def reference_save_model():
    return _CpuModel(257, 3, np.random.default_rng(5))


def _rewrite_through_dropin(src_path, dst_path):
    """Read a PLY with the drop-in plyfile and write it back with it (describe + write)."""
    from plyfile import PlyData, PlyElement

    el = PlyData.read(src_path)["vertex"]
    PlyData([PlyElement.describe(el.data, "vertex")]).write(dst_path)


def test_reference_store_fetch_through_dropin(tmp_path):
    """scene/dataset_readers.py storePly / fetchPly (the reference's code) against ours."""
    xyz, rgb = reference_store_inputs()
    a, b, c = os.path.join(GOLDEN, "ply_reference_store.ply"), str(tmp_path / "ours.ply"), str(tmp_path / "again.ply")
    ply.store_ply(b, xyz, rgb)
    assert open(a, "rb").read() == open(b, "rb").read()
    ref = np.load(os.path.join(GOLDEN, "ply_reference.npz"))
    ra, rb = (ref["fetch_points"], ref["fetch_colors"], ref["fetch_normals"]), ply.fetch_ply(a)
    for x, y in zip(ra, rb):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
    _rewrite_through_dropin(a, c)
    assert open(a, "rb").read() == open(c, "rb").read()


def test_reference_save_ply_through_dropin(tmp_path):
    """GaussianModel.save_ply (the reference's code, CPU tensors) writes the same bytes as
    ply.save_ply, and plyfile.PlyData.read sees what load_ply expects."""
    src = reference_save_model()
    a, b, c = os.path.join(GOLDEN, "ply_reference_save.ply"), str(tmp_path / "ours.ply"), str(tmp_path / "again.ply")
    ply.save_ply(src, b)
    assert open(a, "rb").read() == open(b, "rb").read()
    ref = np.load(os.path.join(GOLDEN, "ply_reference.npz"))
    assert list(ref["attributes"]) == ply.construct_list_of_attributes(src)
    from plyfile import PlyData

    pd = PlyData.read(a)
    el = pd.elements[0]
    assert len(el) == 257 and el["f_rest_44"].dtype == np.float32
    np.testing.assert_array_equal(el["f_rest_44"], src._features_rest.numpy()[:, 14, 2])
    assert [p.name for p in el.properties] == ply.construct_list_of_attributes(src)
    _rewrite_through_dropin(a, c)
    assert open(a, "rb").read() == open(c, "rb").read()

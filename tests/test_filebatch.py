"""CPU tests of the staged file read both folder loaders share (gmr_amd._filebatch), with a plain torch.empty allocator in place of the
loaders' page-locked cache: packing, skip_errors, the per-format parsers' error rules and the read-ahead order."""
import glob
import os
import re
import struct
import threading

import numpy as np
import pytest
import torch

from gmr_amd import _filebatch as fb
from gmr_amd.bvh import _header, read_bvh
from gmr_amd.smplx_adapter import _joint_meta, save_joint_file

ALLOC = lambda n: torch.empty(n, dtype=torch.uint8)
JOINT = lambda view, path: _joint_meta(view, path, 55)


def _joint_file(path, T=5):
    save_joint_file(path, np.zeros((T, 55, 3), np.float32), np.zeros((T, 3), np.float32), np.zeros((T, 165), np.float32), 30.0, np.zeros(16))
    return str(path)


def test_read_files_packs_every_file_on_its_boundary(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "bvh_*.bvh")))
    for align, parse in ((64, _header), (256, lambda view, path: bytes(view))):
        st = fb.read_files(files, ALLOC, align, parse, 3, False)
        host = st.buf.numpy()
        assert st.files == files and st.skipped == [] and len(st.parsed) == len(files)
        assert all(s % align == 0 for s in st.starts) and st.starts[0] == 0
        for f, a, n in zip(files, st.starts, st.sizes):
            raw = open(f, "rb").read()
            assert n == len(raw) and host[a:a + n].tobytes() == raw
        assert st.total == int(st.starts[-1] + (st.sizes[-1] + align - 1) // align * align) and st.buf.numel() >= st.total + align
    # (every golden file passes the header checks and loads, the frame-count bound included)
    assert all(len(read_bvh(f)) == _header(open(f, "rb").read(), f)[1] for f in files)


def test_read_files_skip_errors(golden_dir, tmp_path):
    good = os.path.join(golden_dir, "bvh_lafan_like.bvh")
    junk = tmp_path / "junk.bvh"
    junk.write_text("this is not a BVH file\n")
    ragged = tmp_path / "ragged.bvh"
    ragged.write_bytes(open(good, "rb").read().replace(b"}", b"", 1))   # one joint left open
    missing = str(tmp_path / "missing.bvh")
    for bad, err in ((missing, OSError), (str(junk), ValueError), (str(ragged), ValueError)):
        with pytest.raises(err):
            fb.read_files([good, bad], ALLOC, 64, _header, 2, False)
    st = fb.read_files([good, missing, str(junk), str(ragged), good], ALLOC, 64, _header, 2, True)
    assert st.files == [good, good] and [f for f, _ in st.skipped] == [missing, str(junk), str(ragged)] and all(r for _, r in st.skipped)
    # the skipped files were staged too: one copy of buf[:total] moves the group
    assert st.starts.tolist() == [0, int(st.starts[1])] and st.total > st.starts[1] + st.sizes[1]
    # joint files: a truncated central directory is a malformed file, not a crash of the batch
    ok = _joint_file(tmp_path / "ok.npz")
    raw = open(ok, "rb").read()
    k = raw.rfind(b"PK\x05\x06")
    cd_off = struct.unpack_from("<I", raw, k + 16)[0]
    corrupt = tmp_path / "corrupt.npz"
    corrupt.write_bytes(raw[:cd_off + 20] + raw[k:])
    with pytest.raises(ValueError, match="malformed zip archive"):
        fb.read_files([ok, str(corrupt)], ALLOC, 256, JOINT, 2, False)
    st = fb.read_files([ok, str(corrupt), str(tmp_path / "none.npz")], ALLOC, 256, JOINT, 2, True)
    assert st.files == [ok] and [f for f, _ in st.skipped] == [str(tmp_path / "none.npz"), str(corrupt)]
    assert st.parsed[0]["T"] == 5 and st.parsed[0]["fps"] == 30.0 and "malformed zip archive" in st.skipped[1][1]


def test_read_files_does_not_swallow_bugs(golden_dir):
    def buggy(view, path):
        raise TypeError("a bug in the parser")
    with pytest.raises(TypeError):
        fb.read_files([os.path.join(golden_dir, "bvh_lafan_like.bvh")], ALLOC, 64, buggy, 1, True)


def test_bvh_frame_count_the_file_cannot_hold(golden_dir, tmp_path):
    raw = open(os.path.join(golden_dir, "bvh_lafan_like.bvh"), "rb").read()
    huge = tmp_path / "huge.bvh"
    huge.write_bytes(re.sub(rb"Frames:\s*\d+", b"Frames: " + str(10 ** 12).encode(), raw))
    with pytest.raises(ValueError, match="frames"):
        read_bvh(str(huge))
    st = fb.read_files([str(huge)], ALLOC, 64, _header, 1, True)
    assert st.files == [] and "10000000000" in st.skipped[0][1]


def test_read_ahead_order_and_slots():
    seen, main = [], threading.get_ident()

    def read(group, slot):
        seen.append((group, slot, threading.get_ident() != main))
        return group, slot
    groups = [["a"], ["b", "c"], ["d"], ["e"]]
    assert list(fb.read_ahead(groups, read, lambda got: got)) == [(g, k & 1) for k, g in enumerate(groups)]
    assert seen == [(g, k & 1, True) for k, g in enumerate(groups)]
    assert list(fb.read_ahead([], read, lambda got: got)) == []

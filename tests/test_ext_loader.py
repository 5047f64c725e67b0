"""The extension loader reuses a prebuilt .so only while it is newer than
every file in csrc/, headers included (shared device code lives in them)."""

import os

from dfno_amd import _ext


def _tree(tmp_path, monkeypatch):
    csrc, build = tmp_path / "csrc", tmp_path / "_build"
    csrc.mkdir()
    build.mkdir()
    src, hdr = csrc / "a.hip", csrc / "util.h"
    src.write_text("// source\n")
    hdr.write_text("// header\n")
    so = build / f"{_ext._EXT_NAME}.so"
    so.write_bytes(b"")
    monkeypatch.setattr(_ext, "_CSRC", csrc)
    monkeypatch.setattr(_ext, "_BUILD", build)
    monkeypatch.setattr(_ext, "SOURCES", [src])   # the header is not listed
    return src, hdr, so


def _set_mtime(path, t):
    os.utime(path, (t, t))


def test_prebuilt_older_than_a_header_is_stale(tmp_path, monkeypatch):
    src, hdr, so = _tree(tmp_path, monkeypatch)
    _set_mtime(src, 1000)
    _set_mtime(so, 2000)
    _set_mtime(hdr, 3000)
    assert _ext._find_prebuilt() is None


def test_prebuilt_newer_than_all_of_csrc_is_used(tmp_path, monkeypatch):
    src, hdr, so = _tree(tmp_path, monkeypatch)
    _set_mtime(src, 1000)
    _set_mtime(hdr, 1500)
    _set_mtime(so, 2000)
    assert _ext._find_prebuilt() == so

"""The C-ABI shared library: it loads without a GPU, exports every symbol that
include/sknnr_hip.h declares, and fails loudly (no CPU fallback) when no device exists."""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "sknnr_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(sknnr_[a-z_0-9]+)\s*\(", text)))


@pytest.fixture(scope="module")
def native():
    from sknnr_amd import _build, _native

    if not os.path.exists(_build.LIB_PATH):
        _build.build()
    _native.load()
    return _native


def test_header_and_binding_agree(native):
    assert declared_functions() == sorted(native.EXPORTED_SYMBOLS)


def test_library_exports_every_declared_symbol(native):
    lib = ctypes.CDLL(native.library_path())
    for name in declared_functions():
        assert hasattr(lib, name), f"{name} is declared in include/sknnr_hip.h but not exported"


def test_no_other_symbols_leak(native):
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only", native.library_path()], capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    exported = {s for s in exported if not s.startswith("_")}
    assert exported == set(declared_functions())


def test_abi_version_and_last_error(native):
    lib = native.load()
    assert lib.sknnr_abi_version() == native.ABI_VERSION == 5
    assert isinstance(lib.sknnr_last_error(), bytes)


def test_struct_layouts_match_the_header(native):
    assert ctypes.sizeof(native.QueryOpts) == 48  # ABI v5: + query_dtype, reserved_
    assert native.QueryOpts.row_offset.offset == 40
    assert native.QueryOpts.check_finite.offset == 28
    assert native.QueryOpts.query_dtype.offset == 32
    # the header's struct, compiled: same size and offsets
    import subprocess, tempfile

    src = '#include <stddef.h>\n#include <stdio.h>\n#include "sknnr_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(sknnr_query_opts), offsetof(sknnr_query_opts, query_dtype), offsetof(sknnr_query_opts, row_offset), sizeof(sknnr_stats));return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "layout.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "layout")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in got] == [48, 32, 40, 88]
    assert ctypes.sizeof(native.Stats) == 88  # ABI v4: + mfma_executed_ratio
    assert native.Stats.total_kernel_ms.offset == 48


def test_argument_errors_without_touching_a_device(native):
    lib = native.load()
    assert lib.sknnr_index_create(None, 10, 3, None, 0, 0, ctypes.byref(ctypes.c_void_p())) == native.ERR_INVALID
    assert b"ref must be" in lib.sknnr_last_error()
    assert lib.sknnr_kneighbors(None, None, 1, None, None, None, 0, None) == native.ERR_INVALID
    assert lib.sknnr_check_finite(None, None) == native.ERR_INVALID
    assert lib.sknnr_stream_begin(None, None, 0, 0, ctypes.byref(ctypes.c_void_p())) == native.ERR_INVALID
    assert lib.sknnr_stream_push(None, None, 1, None, None, None) == native.ERR_INVALID
    assert lib.sknnr_stream_flush(None) == native.ERR_INVALID
    assert lib.sknnr_hamming_distances(None, None, 0, None, 1, None, 0, None) == native.ERR_INVALID
    assert lib.sknnr_debug_coarse_candidates(None, 1, None, None, None) == native.ERR_INVALID
    assert b"NULL" in lib.sknnr_last_error()
    assert lib.sknnr_stream_end(None, None) == 0  # NULL is allowed
    lib.sknnr_index_destroy(None)  # NULL is allowed


@pytest.mark.gpu
def test_coarse_candidates_errors(native):
    """sknnr_debug_coarse_candidates: the lists of the last chunk with its padding rows; INVALID on a NULL output or beyond
    the chunk; UNSUPPORTED after a call that ran no pre-filter, filed merged candidate records or ran the second-generation kernel."""
    from sknnr_amd import synth

    lib = native.load()
    x_ref, _, x_q = synth.make_problem(1_300, 100, 13, t=1)
    ix = native.Index(x_ref)
    try:
        ix.kneighbors_host(x_q, ix.make_opts(5))
        assert ix.debug_last_prefilter()["generation"] == 1 and ix.debug_last_finalize()["record"] == 0
        val, pos, perm = ix.debug_coarse_candidates(6_144)  # the padding rows are the chunk's too
        assert val.shape == pos.shape == (6_144, 2, 6) and sorted(perm.tolist()) == list(range(1_300))
        # (5 neighbours on lists of 6: no sentinel, and 650 rows on either lane half fill both lists of a live row)
        assert (pos[:100] >= 0).all() and (pos[:100] < 1_300).all() and np.isfinite(val[:100]).all()
        with pytest.raises(native.HipBackendError, match="the last device chunk has 6144") as e:
            ix.debug_coarse_candidates(6_145)
        assert e.value.code == native.ERR_INVALID
        for args in ((None, pos, perm), (val, None, perm), (val, pos, None)):
            ptrs = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in args]
            assert lib.sknnr_debug_coarse_candidates(ix.handle, 1, *ptrs) == native.ERR_INVALID
        ix.kneighbors_host(x_q, ix.make_opts(40))  # more neighbours than the pre-filter serves: the exact scan alone
        assert ix.debug_last_prefilter()["generation"] == 0
        with pytest.raises(native.HipBackendError, match="no Euclidean pre-filter") as e:
            ix.debug_coarse_candidates(1)
        assert e.value.code == native.ERR_UNSUPPORTED
    finally:
        ix.close()
    x_ref, _, x_q = synth.make_problem(4_000, 100, 13, t=1)
    ix = native.Index(x_ref)
    try:
        ix.kneighbors_host(x_q, ix.make_opts(5))
        assert ix.debug_last_finalize()["record"] == 1
        with pytest.raises(native.HipBackendError, match="merged candidate records") as e:
            ix.debug_coarse_candidates(1)
        assert e.value.code == native.ERR_UNSUPPORTED
        ix.kneighbors_host(x_q, ix.make_opts(7))  # second-generation lists of 8: filed by position, not served
        assert ix.debug_last_prefilter()["generation"] == 2 and ix.debug_last_finalize()["record"] == 0
        with pytest.raises(native.HipBackendError, match="second-generation") as e:
            ix.debug_coarse_candidates(1)
        assert e.value.code == native.ERR_UNSUPPORTED
    finally:
        ix.close()


@pytest.mark.skipif("__import__('sknnr_amd')._native.device_count() > 0")
def test_fails_loudly_without_a_gpu(native):
    """No CPU fallback: without a device the product path raises."""
    import sknnr_amd

    x = np.random.default_rng(0).standard_normal((20, 4))
    with pytest.raises(native.HipBackendError, match="no HIP device"):
        native.Index(x)
    with pytest.raises(native.HipBackendError, match="no HIP device"):
        sknnr_amd.RawKNNRegressor(n_neighbors=2).fit(x, x[:, :2])
    with pytest.raises(native.HipBackendError, match="no HIP device"):
        sknnr_amd.EuclideanKNNRegressor(n_neighbors=2).fit(x, x[:, :2])

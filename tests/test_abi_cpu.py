"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol
include/zvec_hip.h declares; without a GPU the product path fails loudly (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "zvec_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(zvec_hip_[a-z_0-9]+)\s*\(", text)))


def test_header_and_binding_agree():
    from zvec_amd import _lib
    decl = _declared_symbols()
    assert len(decl) >= 30
    assert sorted(_lib.SYMBOLS) == decl


def test_library_exports_every_declared_symbol():
    from zvec_amd import _lib
    L = _lib.lib()
    for name in _declared_symbols():
        assert hasattr(L, name), name
    assert L.zvec_hip_abi_version() == 1


def test_error_strings_follow_reference_table():
    # src/core/framework/index_error.cc:20-71
    from zvec_amd import _lib
    L = _lib.lib()
    assert L.zvec_hip_error_string(0) == b"Success"
    assert L.zvec_hip_error_string(-31) == b"Invalid argument"
    assert L.zvec_hip_error_string(-12) == b"Unsupported"
    assert L.zvec_hip_error_string(-204) == b"No index loaded"


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import zvec_amd
    with pytest.raises(RuntimeError):
        zvec_amd.HipFlatSearcher(16)
    with pytest.raises(RuntimeError):
        zvec_amd.HipIVFSearcher(16)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "zvec_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cc", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in src.replace("oracle/", "ORACLE_DIR_MENTION").replace("import oracle", "X") or \
                    "import oracle" not in src, f
                assert "from oracle" not in src and "import oracle" not in src and "liboracle" not in src, f


def test_shard_map_is_byte_balanced_and_matches_restatement():
    """zvec_hip_ivf_shard_map is pure host arithmetic (no HIP call): greedy largest-first by 128-row tiles."""
    import numpy as np
    import zvec_amd
    from tests.util import lpt_owner
    rng = np.random.default_rng(3)
    for nlist, nshards in ((48, 3), (4096, 8), (16384, 8), (7, 8), (100, 1)):
        sizes = (rng.gamma(2.0, 1200.0, nlist)).astype(np.uint32)
        sizes[rng.integers(0, nlist, max(1, nlist // 50))] = 0          # some empty lists
        owner, rows = zvec_amd.shard_map(sizes, nshards)
        assert np.array_equal(owner, lpt_owner(sizes, nshards))
        assert int(rows.sum()) == int(sizes.astype(np.uint64).sum())
        for g in range(nshards):
            assert int(rows[g]) == int(sizes[owner == g].astype(np.uint64).sum())
        if nlist >= 64 * nshards:
            tiles = np.array([((sizes[owner == g].astype(np.int64) + 127) // 128).sum() for g in range(nshards)])
            assert tiles.max() <= 1.01 * tiles.mean()                   # balanced by bytes


def test_boundary_a_parameter_mapping_arithmetic():
    """patches/boundary_a.diff hands boundary A's nprobe to IVFSearcherContext::update as scan_ratio = nprobe / nlist
    (ivf_searcher_context.h:61-79): round(nlist * scan_ratio) must give nprobe back for the BASELINE configurations and
    for awkward (non power-of-two) list counts; brute_force_threshold = N - 1 pins max_scan_count at N - 1."""
    import numpy as np
    from zvec_amd.index import ivf_probe_params
    for nlist, nprobe, n in ((4096, 32, 10_000_000), (4096, 38, 10_000_000), (16384, 64, 100_000_000), (1000, 7, 123_457),
                             (1024, 1, 5000), (3, 3, 10), (65536, 1, 1 << 30)):
        ratio = float(np.float32(nprobe) / np.float32(nlist))
        got, max_scan = ivf_probe_params(nlist, n, ratio, n - 1)
        assert got == nprobe and max_scan == max(n - 1, int(np.ceil(np.float32(n) * np.float32(ratio))))
    # the reference defaults (scan_ratio 0.1, threshold 1000, ivf_searcher_context.h:211-213)
    assert ivf_probe_params(1024, 50_000, 0.1, 1000) == (102, 5000)
    assert ivf_probe_params(4, 100, 0.1, 1000) == (1, 1000)


def _segments(image, checksum=1):
    from zvec_amd import _lib
    L = _lib.lib()
    n = C.c_uint32(0)
    rc = L.zvec_hip_container_segments(image, len(image), checksum, None, 0, C.byref(n))
    if rc != 0:
        return rc, []
    arr = (_lib.Segment * n.value)()
    rc = L.zvec_hip_container_segments(image, len(image), checksum, arr, n.value, C.byref(n))
    return rc, [(s.id.decode(), int(s.offset), int(s.size), int(s.padding), int(s.crc)) for s in arr]


def test_container_framing_of_a_dumped_index_file():
    """IndexUnpacker::unpack restated (index_unpacker.h:103-330, index_format.h:26-95) — host-only: segment table of a
    file image written by the restated IndexPacker (tests/ivf_format.py::pack_container); header / footer / meta / content
    checksums verified; corrupt and truncated images refused with the reference's error classes."""
    import numpy as np
    from oracle.roaring import crc32c
    from tests.ivf_format import pack_container
    rng = np.random.default_rng(2)
    segs = [("flat.keys", np.arange(37, dtype=np.uint64).tobytes()), ("flat.features", rng.bytes(37 * 20)),
            ("IndexMeta", rng.bytes(4128)), ("empty.one", b"")]
    image = pack_container(segs)
    rc, got = _segments(image)
    assert rc == 0
    assert [g[0] for g in got] == [s[0] for s in segs] + ["IndexVersion"]
    for (sid, data), (gid, off, size, pad, crc) in zip(segs, got):
        assert image[off:off + size] == data and (size + pad) % 32 == 0 and crc == crc32c(data, 0)
    # too small an output array: count still reported
    from zvec_amd import _lib
    n = C.c_uint32(0)
    arr = (_lib.Segment * 2)()
    assert _lib.lib().zvec_hip_container_segments(image, len(image), 1, arr, 2, C.byref(n)) == -17 and n.value == 5
    # corruption: header byte, footer byte, meta byte -> Mismatch; content byte only with checksum on
    for pos in (8, 40, len(image) - 60, len(image) - 128 - 8):   # header x2, footer (reserved words), segment-id block
        bad = bytearray(image)
        bad[pos] ^= 0x40
        assert _segments(bytes(bad))[0] == -24, pos
    bad = bytearray(image)
    bad[64 + 5] ^= 1
    assert _segments(bytes(bad), checksum=1)[0] == -24 and _segments(bytes(bad), checksum=0)[0] == 0
    assert _segments(image[:-1])[0] in (-24, -31) and _segments(image[:40])[0] == -31


def test_header_is_plain_c_and_a_c_program_links():
    """the boundary is a C ABI: include/zvec_hip.h compiles as C99 (-pedantic), and examples/flat_search.c — a C program
    written against it — compiles and links with the shared library (it needs a GPU to RUN: tests/test_gpu_flat.py does)"""
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = os.path.join(root, "include", "zvec_hip.h")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr])
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "flat_search")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), "-o", exe,
                               os.path.join(root, "examples", "flat_search.c"), "-L" + os.path.join(root, "zvec_amd"), "-lzvec_hip",
                               "-Wl,-rpath," + os.path.join(root, "zvec_amd")])
        assert os.path.exists(exe)


def test_runtime_options_round_trip_without_a_gpu():
    """zvec_hip_set_option / zvec_hip_get_option (include/zvec_hip.h): process-wide switches, no device call behind them — every
    documented name takes its documented range, reads back, refuses values outside it and unknown names."""
    import ctypes as C
    from zvec_amd import _lib
    L = _lib.lib()
    v = C.c_int(-1)
    for name, ok_values, bad in ((b"wait", (0, 1, 2), 3), (b"zerocopy", (0, 1, 2, 3), 4), (b"scan256", (0, 1, 2), 3)):
        assert L.zvec_hip_get_option(name, C.byref(v)) == 0
        before = v.value
        for x in ok_values:
            assert L.zvec_hip_set_option(name, x) == 0
            assert L.zvec_hip_get_option(name, C.byref(v)) == 0 and v.value == x
        assert L.zvec_hip_set_option(name, bad) != 0 and L.zvec_hip_set_option(name, -1) != 0
        assert L.zvec_hip_get_option(name, C.byref(v)) == 0 and v.value == ok_values[-1]
        assert L.zvec_hip_set_option(name, before) == 0
    assert L.zvec_hip_set_option(b"assign256", 0) == 0 and L.zvec_hip_get_option(b"assign256", C.byref(v)) == 0 and v.value == 0
    assert L.zvec_hip_set_option(b"assign256", 1) == 0
    assert L.zvec_hip_set_option(b"no-such-option", 1) != 0 and L.zvec_hip_get_option(b"no-such-option", C.byref(v)) != 0
    assert L.zvec_hip_set_option(None, 1) != 0


def test_route_read_back_validates_its_arguments_without_a_gpu():
    """zvec_hip_ctx_last_route is host bookkeeping: declared, bound and exported (the symbol tests above), and it refuses a null
    context or a null output before touching anything"""
    import ctypes as C
    from zvec_amd import _lib
    L = _lib.lib()
    assert "zvec_hip_ctx_last_route" in _declared_symbols() and "zvec_hip_ctx_last_route" in _lib.SYMBOLS
    r = C.c_uint32(123)
    assert L.zvec_hip_ctx_last_route(None, C.byref(r)) == -31 and r.value == 123
    assert L.zvec_hip_ctx_last_route(None, None) == -31


def test_ivf_plan_read_back_validates_its_arguments_without_a_gpu():
    """zvec_hip_ctx_last_ivf_plan is declared, bound and exported; it refuses a null context or a null info block before touching
    anything, and the ctypes mirror of zvec_hip_ivf_plan_info has the header's fields in the header's order and size"""
    import ctypes as C
    from zvec_amd import _lib
    L = _lib.lib()
    assert "zvec_hip_ctx_last_ivf_plan" in _declared_symbols() and "zvec_hip_ctx_last_ivf_plan" in _lib.SYMBOLS
    info = _lib.IvfPlanInfo()
    info.route, info.slots_bound = 77, 5
    nulls = [None] * 10
    assert L.zvec_hip_ctx_last_ivf_plan(None, C.byref(info), *nulls) == -31 and info.route == 77 and info.slots_bound == 5
    assert L.zvec_hip_ctx_last_ivf_plan(None, None, *nulls) == -31
    text = open(os.path.join(ROOT, "include", "zvec_hip.h")).read()
    body = re.search(r"typedef struct zvec_hip_ivf_plan_info \{(.*?)\} zvec_hip_ivf_plan_info;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(uint32_t|uint64_t)\s+([a-z_, ]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert fields == [(n, "uint64_t" if t is C.c_uint64 else "uint32_t") for n, t in _lib.IvfPlanInfo._fields_]
    assert C.sizeof(_lib.IvfPlanInfo) == 4 * 10 + 8
    routes = dict(re.findall(r"#define ZVEC_HIP_IVF_ROUTE_([A-Z_]+) (\d)u", text))
    assert {k: int(v) for k, v in routes.items()} == {
        "NONE": _lib.IVF_ROUTE_NONE, "DIRECT_BLOCK_TOPK": _lib.IVF_ROUTE_DIRECT_BLOCK_TOPK, "DIRECT_SELECT": _lib.IVF_ROUTE_DIRECT_SELECT,
        "TILE": _lib.IVF_ROUTE_TILE, "LARGE_K": _lib.IVF_ROUTE_LARGE_K}
    assert re.search(r"ZVEC_HIP_ERR_NO_READY = (-\d+)", text).group(1) == str(_lib.ERR_NO_READY)


def test_shadow_entry_points_refuse_null_handles_without_a_gpu():
    """the half-width pre-selection entry points (zvec_hip_ivf_set_shadow / zvec_hip_flat_set_shadow and their _info / _certify
    companions) validate their arguments before any device call"""
    import ctypes as C
    from zvec_amd import _lib
    L = _lib.lib()
    n = C.c_uint32(5)
    on = C.c_int(7)
    for pre in ("zvec_hip_ivf", "zvec_hip_flat"):
        assert getattr(L, pre + "_set_shadow")(None, 1, 0) == -31
        assert getattr(L, pre + "_shadow_info")(None, C.byref(on), None, None, None) == -31
    assert L.zvec_hip_ivf_shadow_certify(None, None, None, 1, 1, 1, 1, None, None, None, None, None, C.byref(n)) == -31
    assert L.zvec_hip_flat_shadow_certify(None, None, None, 1, 1, None, None, None, None, None, C.byref(n)) == -31

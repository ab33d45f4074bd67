"""The C++ drop-in host layer (stereo_matching_cuda_amd/host/: main.cpp + the reference's per-stage
headers) built against libsmx_hip.so.  CPU: it builds, keeps the reference's function names, and
fails loudly without a GPU.  GPU: running the drop-in main on the reference's Tsukuba pair writes
12 PNGs whose pixels equal the 12 PNGs the reference's authors committed.
The CPU twins of the opt-in stages (SGM, speckle removal, weighted median) are held to their numpy references, plain and
under the sanitizers, in tests/test_host_twins_cpu.py; the main's --aggregation sgm path in tests/test_gpu_main_sgm.py."""
import os
import re
import subprocess

import numpy as np
import pytest

from main_harness import binary  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "stereo_matching_cuda_amd", "host")

REFERENCE_SIGNATURES = {   # reference header -> host function names it must still declare
    "rgb_to_grayscale.cuh": ["rgb_to_grayscale", "sumArraysOnHost", "check_errors_grayscale"],
    "costVolume.cuh": ["compute_cost", "costVolumeOnCPU", "x_derivativeCPU", "iDivUp",
                       "compute_costVolumeOnCpu", "x_derivativeOnCpu"],
    "guidedFilter.cuh": ["compute_guided_filter", "dispSelectOnCPU", "computeBoxFilterOnCPU",
                         "computeMeanOnCPU", "chToFlOnCPU", "flToChOnCPU", "pixelMultOnCPU",
                         "pixelSousOnCPU", "pixelAddOnCPU", "pixelDivOnCPU", "guided_filter_onCpu"],
    "integral.cuh": ["integral", "integralOnCPU"],
    "occlusion.cuh": ["detect_occlusion", "fill_occlusion", "detect_occlusionOnCPU", "fill_occlusionOnCPU"],
    "filter.cuh": ["filter", "boxFilterOnCPU"],
    "helpers.cuh": ["check_errors"],
    "winner_take_all.cuh": ["wta_pack"],
}

OUTPUTS = ["image_left", "image_right", "image_mean_left", "image_mean_right", "best_costl",
           "best_costr", "cost_lminus15", "cost_rminus15", "occlu_mapl", "disparity_mapl",
           "disparity_mapr", "occlu_mapl_filled"]


def test_headers_keep_the_reference_names():
    for header, names in REFERENCE_SIGNATURES.items():
        src = open(os.path.join(HOST, header)).read()
        for n in names:
            assert re.search(r"\b%s\s*\(" % n, src), (header, n)


def test_host_layer_builds_and_links_the_c_abi(binary):
    out = subprocess.run(["ldd", binary], capture_output=True, text=True).stdout
    assert "libsmx_hip.so" in out


def test_main_fails_loudly_without_gpu(binary, tmp_path):
    import stereo_matching_cuda_amd as smx
    if smx.lib().smx_device_count() > 0:
        pytest.skip("a GPU is present")
    r = subprocess.run([binary], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode != 0 and "no HIP device" in r.stderr


def _build(out, sources, shared=False):
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + HOST]
    lib = os.path.join(ROOT, "stereo_matching_cuda_amd", "_build")
    cmd = (["g++", "-O2", "-std=c++17", "-ffp-contract=off"] + (["-shared", "-fPIC"] if shared else []) + inc +
           sources + ["-o", out, "-L" + lib, "-lsmx_hip", "-lz", "-Wl,-rpath," + lib])
    subprocess.check_call(cmd)
    return out


def test_cpu_twins_of_the_host_compare_mode_equal_the_oracle(binary, golden, orc, tmp_path):
    """The CPU twins behind host_gpu_compare (host/cpu_twins.cpp; reference declarations
    costVolume.cuh:8-14, guidedFilter.cuh:9-39, integral.cuh:7, occlusion.cuh:12,19) are product code:
    hold them against the oracle on a Tsukuba crop, no GPU needed."""
    import ctypes as C
    so = _build(str(tmp_path / "libtwins.so"),
                [os.path.join(ROOT, "tests", "host_twins_capi.cpp"), os.path.join(HOST, "cpu_twins.cpp"),
                 os.path.join(HOST, "stages.cpp")], shared=True)
    T = C.CDLL(so)
    vp = C.c_void_p
    def ptr(a):
        return a.ctypes.data_as(vp)
    rgb = np.ascontiguousarray(golden["tsukuba0"][60:130, 100:200])
    rgb2 = np.ascontiguousarray(golden["tsukuba1"][60:130, 100:200])
    h, w = rgb.shape[:2]
    g1 = np.empty((h, w), np.uint8); g2 = np.empty((h, w), np.uint8)
    T.twin_gray(ptr(rgb), ptr(g1), h * w, rgb.shape[2])
    T.twin_gray(ptr(rgb2), ptr(g2), h * w, rgb2.shape[2])
    assert np.array_equal(g1, orc.gray(rgb)) and np.array_equal(g2, orc.gray(rgb2))
    D, dmin = 6, -5
    cost = np.empty((D, h, w), np.float32)
    T.twin_cost(ptr(g1), ptr(g2), ptr(cost), w, h, D, dmin)
    want_cost = orc.cost_volume(g1, g2, D, dmin)
    assert np.array_equal(cost.view(np.uint32), want_cost.view(np.uint32))
    S = np.empty((h, w), np.float32)
    T.twin_integral(ptr(cost[2]), ptr(S), w, h)
    assert np.array_equal(S.view(np.uint32), orc.integral(cost[2]).view(np.uint32))
    best, dmap = orc.init_wta(h, w)
    mean = np.empty((h, w), np.uint8)
    T.twin_guided(ptr(g1), ptr(cost), ptr(best), ptr(dmap), ptr(mean), w, h, D, dmin)
    wb, wd, wm, _ = orc.guided_filter(g1, want_cost, dmin)
    assert np.array_equal(best.view(np.uint32), wb.view(np.uint32))
    assert np.array_equal(dmap, wd) and np.array_equal(mean, wm)
    dr = np.abs(dmap[:, ::-1]).copy()
    occ = dmap.copy()
    T.twin_detect(ptr(occ), ptr(dr), dmin - 100, w, h)
    want_occ = orc.detect_occlusion(dmap, dr, dmin - 100)
    assert np.array_equal(occ, want_occ)
    T.twin_fill(ptr(occ), w, h, C.c_float(float(dmin)))
    assert np.array_equal(occ, orc.fill_occlusion(want_occ, float(dmin)))


@pytest.mark.gpu
def test_reference_signature_wrappers_on_the_gpu(binary, tmp_path):
    """integral(), filter(), check_errors(), detect/fill_occlusion of host/*.cuh called from C++."""
    exe = _build(str(tmp_path / "wrappers_check"),
                 [os.path.join(ROOT, "tests", "host_wrappers_check.cpp"), os.path.join(HOST, "cpu_twins.cpp"),
                  os.path.join(HOST, "stages.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("check_errors", "integral", "filter", "boxFilterOnCPU", "occlusion"):
        assert "ok " + name in r.stdout, r.stdout


def _stage_tsukuba(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    for n in ("tsukuba0", "tsukuba1"):
        src = os.path.join(ROOT, "tests", "golden", "tsukuba", n + ".png")
        (data / (n + ".png")).write_bytes(open(src, "rb").read())
    return data


@pytest.mark.gpu
def test_drop_in_main_fast_mode(binary, golden, tmp_path):
    """--fast (the non-bit-exact aggregation): runs, writes the 12 images, and differs from the
    committed disparity maps in a handful of labels only."""
    PIL = pytest.importorskip("PIL.Image")
    data = _stage_tsukuba(tmp_path)
    r = subprocess.run([binary, "--fused", "--fast"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("disparity_mapl", "disparity_mapr"):
        got = np.asarray(PIL.open(data / (name + ".png")))
        diff = int((got != golden[name]).sum())
        print(name, "pixels that differ from the committed image:", diff)
        assert diff < 200, (name, diff)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [["--fused"], ["--host-compare"], ["--fused", "--host-compare"],
                                   ["--ngpu", "1"], ["--fused", "--pairs", "4"], ["--fused", "--pairs", "5", "--pipeline"],
                                   ["--ngpu", "1", "--pairs", "3"],
                                   ["--ngpu", "1", "--overlap", "--pairs", "3"]])
def test_drop_in_main_modes(binary, golden, tmp_path, flags):
    """--fused: one device-resident call after the gray conversion; --host-compare: the reference's
    self-check mode (main.cu:40) with correct CPU twins; --ngpu 1: the RCCL sharded driver of
    libsmx_rccl.so with a one-rank communicator (the N > 1 call sequence on the one GPU of this box);
    --pairs K: K pairs on ONE persistent context (smx_create / smx_sharded_create: nothing allocated per
    pair); --overlap: one launch per view, the exchange of the left keys on its own stream.
    Same 12 images every way."""
    PIL = pytest.importorskip("PIL.Image")
    data = _stage_tsukuba(tmp_path)
    pfm = tmp_path / "d.pfm"
    p16 = tmp_path / "d.png"
    r = subprocess.run([binary] + flags + ["--pfm", str(pfm), "--png16", str(p16)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "error at element" not in r.stdout
    if "--pairs" in flags:
        assert re.search(r"pairs \d+ on one context: [0-9.]+ ms per pair", r.stdout), r.stdout
    if "--host-compare" in flags:
        assert "Grayscale ok!" in r.stdout
        assert ("Occlusion ok!" if "--fused" in flags else "Guided filter ok!") in r.stdout
    for name in OUTPUTS:
        got = np.asarray(PIL.open(data / (name + ".png")))
        assert np.array_equal(got, golden[name]), name
        # not only the pixels -- the FILES equal the reference's own outputs byte for byte (main.cu:162-181
        # writes them through stb_image_write; host/png_io.cpp restates that writer's filter and match decisions)
        ref = open(os.path.join(ROOT, "tests", "golden", "tsukuba", name + ".png"), "rb").read()
        assert (data / (name + ".png")).read_bytes() == ref, name
    # dataset-style outputs: positive disparities of the filled left map
    raw = pfm.read_bytes()
    head, rest = raw.split(b"\n", 3)[:3], raw.split(b"\n", 3)[3]
    assert head[0] == b"Pf" and head[1] == b"384 288" and float(head[2]) < 0
    d = np.frombuffer(rest, "<f4").reshape(288, 384)[::-1]
    assert d.min() >= 0 and d.max() <= 15
    d16 = np.asarray(PIL.open(p16))
    assert d16.dtype in (np.uint16, np.int32) and np.array_equal(d16.astype(np.float32), d * 256.0)


def test_rccl_library_exports_the_exchange_step():
    """include/smx_rccl.h: the C-ABI of the multi-GPU exchange (declared in host/winner_take_all.cuh)."""
    so = os.path.join(ROOT, "stereo_matching_cuda_amd", "_build", "libsmx_rccl.so")
    assert os.path.exists(so), "libsmx_rccl.so not built (make -C stereo_matching_cuda_amd/csrc)"
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True).stdout
    hdr = open(os.path.join(ROOT, "include", "smx_rccl.h")).read()
    for name in ("smx_wta_allreduce", "smx_wta_reduce", "smx_stereo_pair_sharded", "smx_sharded_create",
                 "smx_sharded_run", "smx_sharded_destroy"):
        assert re.search(r"\bT %s\b" % name, syms), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert "smx_wta_allreduce" in open(os.path.join(HOST, "winner_take_all.cuh")).read()


def test_main_rejects_bad_arguments(binary, tmp_path):
    import stereo_matching_cuda_amd as smx
    r = subprocess.run([binary, "--nonsense"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 2 and "unknown option" in r.stderr
    if smx.lib().smx_device_count() > 0:
        r = subprocess.run([binary, "a.png", "b.png", "5", "-5"], cwd=tmp_path, capture_output=True, text=True)
        assert r.returncode == 2 and "bad disparity range" in r.stderr


@pytest.mark.gpu
def test_main_reports_unwritable_output_directory(binary, tmp_path):
    data = _stage_tsukuba(tmp_path)
    r = subprocess.run([binary, str(data / "tsukuba0.png"), str(data / "tsukuba1.png"), "-3", "0",
                        str(tmp_path / "missing_dir")], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "could not be written" in r.stderr


def test_png_writer_reproduces_the_reference_files_byte_for_byte(tmp_path):
    """SURVEY 8 f1 on the CPU: each of the twelve PNGs the reference wrote for Tsukuba (tests/golden/tsukuba, main.cu:162-181
    through its vendored stb_image_write) is decoded and written again by host/png_io.cpp; the new file must `cmp` equal.
    A PNG is not canonical in its pixels -- this pins the row-filter choice (minimum sum of |signed byte|, first on ties),
    the three-byte hash chains cut from 16 to their newer 8, the one lazy step and the fixed-Huffman block."""
    exe = str(tmp_path / "reencode")
    src = tmp_path / "reencode.cpp"
    src.write_text('#include "png_io.h"\n#include <cstdlib>\n'
                   'int main(int c, char** v) { int w, h, ch; unsigned char* p = smx_png_load(v[1], &w, &h, &ch);'
                   ' if (!p) return 2; int ok = smx_png_write(v[2], w, h, ch, p); std::free(p); return ok ? 0 : 3; }\n')
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + HOST, str(src), os.path.join(HOST, "png_io.cpp"),
                           "-o", exe, "-lz"])
    gdir = os.path.join(ROOT, "tests", "golden", "tsukuba")
    assert len(OUTPUTS) == 12
    for name in OUTPUTS:
        ref = os.path.join(gdir, name + ".png")
        out = tmp_path / (name + ".png")
        subprocess.check_call([exe, ref, str(out)])
        assert out.read_bytes() == open(ref, "rb").read(), name
    # a few synthetic shapes through the writer and back through the reader (rows of one pixel, RGB, RGBA, runs > 258)
    rt = tmp_path / "roundtrip.cpp"
    rt.write_text('#include "png_io.h"\n#include <cstdlib>\n#include <cstring>\n#include <vector>\n'
                  'int main() { const int shapes[][3] = {{1,1,1},{1,7,3},{5,1,4},{700,3,1},{33,29,2},{64,64,3}};'
                  ' for (auto& s : shapes) { int w = s[0], h = s[1], ch = s[2]; std::vector<unsigned char> a((size_t)w*h*ch);'
                  ' unsigned x = 12345u + w; for (size_t i = 0; i < a.size(); ++i) { x = x * 1664525u + 1013904223u;'
                  ' a[i] = (i / 97) % 3 == 0 ? 7 : (unsigned char)(x >> 24); }'
                  ' if (!smx_png_write("rt.png", w, h, ch, a.data())) return 1; int W, H, C;'
                  ' unsigned char* p = smx_png_load("rt.png", &W, &H, &C); if (!p || W != w || H != h || C != ch ||'
                  ' std::memcmp(p, a.data(), a.size())) return 2; std::free(p); } return 0; }\n')
    exe2 = str(tmp_path / "roundtrip")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + HOST, str(rt), os.path.join(HOST, "png_io.cpp"),
                           "-o", exe2, "-lz"])
    assert subprocess.run([exe2], cwd=tmp_path).returncode == 0


def test_png_reader_rejects_malformed_files(tmp_path):
    """host/png_io.cpp trusts nothing: truncated IHDR, absurd dimensions, missing IDAT."""
    import struct
    import zlib
    exe = str(tmp_path / "pngcheck")
    src = tmp_path / "pngcheck.cpp"
    src.write_text('#include "png_io.h"\n#include <cstdio>\n#include <cstdlib>\n'
                   'int main(int c, char** v) { int w, h, ch; unsigned char* p = smx_png_load(v[1], &w, &h, &ch);'
                   ' std::printf("%s\\n", p ? "loaded" : "rejected"); std::free(p); return 0; }\n')
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + HOST, str(src), os.path.join(HOST, "png_io.cpp"),
                           "-o", exe, "-lz"])
    sig = b"\x89PNG\r\n\x1a\n"
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    good_ihdr = struct.pack(">IIBBBBB", 2, 2, 8, 0, 0, 0, 0)
    idat = zlib.compress(b"\x00\x01\x02\x00\x03\x04")
    cases = {
        "ok.png": (sig + chunk(b"IHDR", good_ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b""), "loaded"),
        "short_ihdr.png": (sig + chunk(b"IHDR", good_ihdr[:5]) + chunk(b"IEND", b""), "rejected"),
        "huge.png": (sig + chunk(b"IHDR", struct.pack(">IIBBBBB", 0x7FFFFFFF, 0x7FFFFFFF, 8, 0, 0, 0, 0)) +
                     chunk(b"IDAT", idat) + chunk(b"IEND", b""), "rejected"),
        "negative.png": (sig + chunk(b"IHDR", struct.pack(">IIBBBBB", 0xFFFFFFF0, 2, 8, 0, 0, 0, 0)) +
                         chunk(b"IDAT", idat) + chunk(b"IEND", b""), "rejected"),
        "no_idat.png": (sig + chunk(b"IHDR", good_ihdr) + chunk(b"IEND", b""), "rejected"),
        "idat_first.png": (sig + chunk(b"IDAT", idat) + chunk(b"IHDR", good_ihdr) + chunk(b"IEND", b""), "rejected"),
        "truncated.png": (sig + chunk(b"IHDR", good_ihdr)[:-3], "rejected"),
    }
    for name, (blob, want) in cases.items():
        f = tmp_path / name
        f.write_bytes(blob)
        out = subprocess.run([exe, str(f)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == want, (name, out.stdout, out.stderr)


def _write_mat_cases():
    """{name: (map f32, the 8-bit image expected of it)}: every kept wm case of oracle/ref_cases.py with what the reference's
    own write_mat made of it, and the constant map, which the reference defines nothing for (oracle/REF_CASES.md) and the
    project defines as all zeros."""
    import ref_fixtures as rf
    from oracle import ref_cases as rc
    out = {}
    for name in rf.names("wm"):
        c, fx = rf.load(name)
        out[name] = (rf.inputs(c)["mat"], fx["u8"].ravel())
    mat = rc.inputs(rc.BY_NAME["wm_constant"])["mat"]
    assert "wm_constant" not in out and mat.size > 1 and mat.min() == mat.max()
    out["wm_constant"] = (mat, np.zeros(mat.size, np.uint8))
    return out


def test_the_three_normalisers_give_the_reference_bytes(orc):
    """smx.write_mat and oracle.write_mat_u8 on every map of _write_mat_cases, byte for byte (normalise_like_reference of
    host/helpers.cuh and the oracle's C function run on the same maps in the sanitizer test below)."""
    import stereo_matching_cuda_amd as smx
    for name, (mat, want) in _write_mat_cases().items():
        for what, fn in (("smx.write_mat", smx.write_mat), ("oracle.write_mat_u8", orc.write_mat_u8)):
            got = fn(mat)
            assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), (name, what)
            assert fn(mat.reshape(1, -1)).shape == (1, mat.size)


def test_host_layer_and_oracle_under_sanitizers(tmp_path):
    """SURVEY 5 (sanitizers): the CPU twins of host/cpu_twins.cpp, the PNG / PFM code of host/png_io.cpp and the
    oracle, all compiled with -fsanitize=address,undefined (-fno-sanitize-recover): the twins equal the oracle
    bit for bit on a seeded pair, the PNG reader survives malformed files, and no sanitizer report appears.
    The float -> 8-bit normaliser of host/helpers.cuh runs there on every recorded map of the reference's write_mat
    (tests/golden/ref_cases/wm_*.npz) and on the constant map the reference defines nothing for (all zeros here), and
    smx.write_mat and the oracle's write_mat_u8 are held to the same bytes.
    CPU only (no GPU sanitizer runs on this pool)."""
    import shutil
    import struct
    import zlib
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "sanitize_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
    obj = str(tmp_path / "oracle.o")
    san.append("-fsanitize=float-cast-overflow")          # (not part of `undefined`: NaN or an infinity converted to int)
    subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-c", os.path.join(ROOT, "oracle", "smx_oracle.c"), "-o", obj] + san)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_sanitize_check.cpp"), os.path.join(HOST, "cpu_twins.cpp"),
                           os.path.join(HOST, "png_io.cpp"), obj, "-o", exe, "-lz"] + san)
    sig = b"\x89PNG\r\n\x1a\n"
    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    ihdr = struct.pack(">IIBBBBB", 2, 2, 8, 0, 0, 0, 0)
    idat = zlib.compress(b"\x00\x01\x02\x00\x03\x04")
    cases = {
        "ok.png": (sig + chunk(b"IHDR", ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b""), "loaded"),
        "short_ihdr.png": (sig + chunk(b"IHDR", ihdr[:5]) + chunk(b"IEND", b""), "rejected"),
        "huge.png": (sig + chunk(b"IHDR", struct.pack(">IIBBBBB", 0x7FFFFFFF, 0x7FFFFFFF, 8, 0, 0, 0, 0)) +
                     chunk(b"IDAT", idat) + chunk(b"IEND", b""), "rejected"),
        "short_idat.png": (sig + chunk(b"IHDR", struct.pack(">IIBBBBB", 64, 64, 8, 2, 0, 0, 0)) + chunk(b"IDAT", idat) +
                           chunk(b"IEND", b""), "rejected"),
        "bad_filter.png": (sig + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(b"\x09\x01\x02\x07\x03\x04")) +
                           chunk(b"IEND", b""), None),
        "garbage_idat.png": (sig + chunk(b"IHDR", ihdr) + chunk(b"IDAT", b"\x00" * 40) + chunk(b"IEND", b""), "rejected"),
        "truncated.png": (sig + chunk(b"IHDR", ihdr)[:-3], "rejected"),
        "chunk_len_overflow.png": (sig + struct.pack(">I", 0xFFFFFFF0) + b"IHDR" + ihdr, "rejected"),
    }
    files = []
    for name, (blob, _) in cases.items():
        (tmp_path / name).write_bytes(blob)
        files.append(str(tmp_path / name))
    wm = _write_mat_cases()
    assert len(wm) >= 7 and "wm_constant" in wm
    (tmp_path / "wm").mkdir()
    (tmp_path / "wm" / "list.txt").write_text("\n".join(wm) + "\n")
    for name, (mat, want) in wm.items():
        mat.tofile(tmp_path / "wm" / (name + ".f32"))
        want.tofile(tmp_path / "wm" / (name + ".u8"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(tmp_path)] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "MISMATCH" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    for what in ("gray", "cost volume", "integral", "guided filter best", "guided filter dmap", "guided filter mean",
                 "detect occlusion", "fill occlusion", "png round trip"):
        assert "ok " + what in r.stdout, r.stdout
    for name, (_, want) in cases.items():
        if want:
            assert f"{want} {tmp_path / name}" in r.stdout, (name, r.stdout)
    for name in wm:
        assert f"ok write_mat {name}\n" in r.stdout and f"ok oracle write_mat {name}\n" in r.stdout, (name, r.stdout)


@pytest.mark.gpu
def test_drop_in_main_reproduces_the_committed_images(binary, golden, tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    data = _stage_tsukuba(tmp_path)
    r = subprocess.run([binary], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("Starting...", "Resolution : 384x288", "RGB to grayscale ...", "Cost Volume ...",
                 "guided filter ...", "guided filter ok", "writing images ...", "duration:",
                 "Free the memory ..."):
        assert line in r.stdout, line                      # main.cu:41-186 progress lines
    for name in OUTPUTS:
        got = np.asarray(PIL.open(data / (name + ".png")))
        assert np.array_equal(got, golden[name]), name

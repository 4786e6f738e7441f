"""lesson1's corner extraction in the C ABI: declared in the header, exported by the built library, refused without a handle,
a 32-byte record -- and the C++ adapter over it (lslam::LaserScanFeaturesGpu, include/lslam_adapters.hpp) compiles stand-alone
with g++ and links against liblslam_gpu.so.  No device needed; on a GPU box the little program also runs a batch."""
import pathlib
import re
import subprocess

import pytest

import adapter_demo
from lslam_amd import api

ROOT = pathlib.Path(__file__).resolve().parent.parent
SYMBOLS = {
    "lslam_features_create": r"int\s+lslam_features_create\s*\(\s*lslam_context\s*\*",
    "lslam_features_destroy": r"void\s+lslam_features_destroy\s*\(\s*lslam_features\s*\*",
    "lslam_features_set_threshold": r"int\s+lslam_features_set_threshold\s*\(\s*lslam_features\s*\*",
    "lslam_features_batch": r"int\s+lslam_features_batch\s*\(\s*lslam_features\s*\*",
    "lslam_features_batch_dev": r"int\s+lslam_features_batch_dev\s*\(\s*lslam_features\s*\*",
    "lslam_features_stats": r"int\s+lslam_features_stats\s*\(\s*const\s+lslam_features\s*\*",
}


def test_new_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "lslam_gpu.h").read_text()
    L = api.lib()
    for name, decl in SYMBOLS.items():
        assert re.search(r"\b" + decl, header), name
        assert hasattr(L, name), name
    assert L.lslam_abi_version() == 5
    assert "#define LSLAM_ABI_VERSION 5" in header
    for macro, value in (("LSLAM_FEATURE_SECTORS", 6), ("LSLAM_FEATURE_PICKS", 20), ("LSLAM_FEATURE_MAX_READINGS", 1500)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", header), macro
    assert (api.FEATURE_SECTORS, api.FEATURE_PICKS, api.FEATURE_MAX_READINGS) == (6, 20, 1500)
    assert "higher compacted index ranks" in re.sub(r"[\s*/]+", " ", header).lower()  # the tie rule is stated


def test_calls_without_a_handle_are_refused():
    L = api.lib()
    assert L.lslam_features_create(None, None) == -1  # LSLAM_ERR_INVALID_ARGUMENT
    assert L.lslam_features_set_threshold(None, 1.0) == -1
    assert L.lslam_features_stats(None, None) == -1
    for fn in (L.lslam_features_batch, L.lslam_features_batch_dev):
        assert fn(None, 0, 0, None, 0, None, None, None, None) == -1
        assert fn(None, 1, 1081, None, 1081, None, None, None, None) == -1
    L.lslam_features_destroy(None)  # a no-op


def test_the_record_is_32_bytes(tmp_path):
    assert api.FEATURE_RECORD.itemsize == 32
    assert api.FEATURE_RECORD.fields["per_sector"][1] == 8
    src = tmp_path / "rec.c"
    src.write_text('#include <stddef.h>\n#include "lslam_gpu.h"\n'
                   '_Static_assert(sizeof(lslam_feature_record) == 32, "32 bytes");\n'
                   '_Static_assert(offsetof(lslam_feature_record, per_sector) == 8, "per_sector at 8");\n'
                   'int main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-I", str(ROOT / "include"), "-fsyntax-only", str(src)], check=True)


SRC = r'''
#include <cstdio>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "lslam_adapters.hpp"
int main(int argc, char**) {
  lslam_context* ctx = nullptr;
  int rc = lslam_create(0, &ctx);
  if (rc != LSLAM_OK) { std::printf("no device: %s\n", lslam_last_error(nullptr)); return argc > 1 ? 1 : 0; }
  int bad = 0;
  {
    const int n = 360, B = 3;
    std::vector<float> ranges((size_t)B * n);
    for (int k = 0; k < B; k++)
      for (int i = 0; i < n; i++) {  // a square room, 6 m a side, seen from three places, with a few beams lost
        double a = -3.14159265358979 + i * (2.0 * 3.14159265358979 / n), c = std::cos(a), s = std::sin(a);
        double tx = ((c > 0 ? 3.0 : -3.0) - 0.4 * k) / c, ty = ((s > 0 ? 3.0 : -3.0) - 0.3 * k) / s;
        ranges[(size_t)k * n + i] = (float)std::fmin(tx, ty);
        if ((i + 7 * k) % 53 == 0) ranges[(size_t)k * n + i] = std::numeric_limits<float>::infinity();
      }
    std::vector<float> corners((size_t)B * n), one(n);
    std::vector<int32_t> index((size_t)B * 120), i1(120);
    std::vector<lslam_feature_record> rec(B);
    lslam_feature_record r1;
    lslam::LaserScanFeaturesGpu features(ctx, 0.01f);
    features.ScanCallbacks(B, n, ranges.data(), n, corners.data(), index.data(), rec.data());
    for (int k = 0; k < B; k++) {  // every scan of the batch == the one-scan call, bit for bit
      features.ScanCallback(ranges.data() + (size_t)k * n, n, one.data(), i1.data(), &r1);
      bad += std::memcmp(one.data(), corners.data() + (size_t)k * n, n * sizeof(float)) != 0;
      bad += std::memcmp(i1.data(), index.data() + (size_t)k * 120, 120 * sizeof(int32_t)) != 0;
      bad += std::memcmp(&r1, &rec[k], sizeof r1) != 0;
      int shown = 0;
      for (int i = 0; i < n; i++) shown += one[i] != 0.0f;
      std::printf("scan %d: %d finite beams, %d corners (%d in the image)\n", k, r1.n_valid, r1.n_corners, shown);
      bad += shown != r1.n_corners || r1.n_corners < 4 || r1.n_valid >= n;
    }
    features.ScanCallback(ranges.data(), n, one.data());  // without the optional outputs
    bad += std::memcmp(one.data(), corners.data(), n * sizeof(float)) != 0;
    int64_t st[4];
    features.stats(st);
    std::printf("features: %lld scans, %lld launches, %lld growths, %lld waits\n", (long long)st[0], (long long)st[1],
                (long long)st[2], (long long)st[3]);
    bad += st[0] != 2 * B + 1 || st[1] != B + 2;
    bool threw = false;
    try {
      std::vector<float> big(1501, 1.0f), out(1501);
      features.ScanCallback(big.data(), 1501, out.data());
    } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
    threw = false;
    try {
      lslam::LaserScanFeaturesGpu negative(ctx, -1.0f);
    } catch (const std::exception&) { threw = true; }
    if (!threw) bad += 100;
  }
  lslam_destroy(ctx);
  std::printf("features adapter %s\n", bad ? "BAD" : "ok");
  return bad ? 3 : 0;
}
'''


def test_features_adapter_compiles_and_links(tmp_path):
    exe = adapter_demo.build(tmp_path, "features_demo", SRC)
    r = adapter_demo.run(exe)
    assert r.returncode == 0, r.stdout + r.stderr  # without a GPU it reports "no device" and exits 0


@pytest.mark.gpu
def test_features_adapter_runs_on_gpu(tmp_path):
    exe = adapter_demo.build(tmp_path, "features_demo", SRC)
    r = adapter_demo.run(exe, "need-gpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "features adapter ok" in r.stdout

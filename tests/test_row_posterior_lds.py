"""The dynamic-LDS carves of csrc/row_posterior.h (CPU only: a small host program is compiled against the header).

The summary, population and level kernels carve their LDS with one builder.  Its byte totals are compared with the
four formulas the kernels used before they shared it, written out here as plain arithmetic, and with the figures the
sources quote: 51,792 B (32 x 32 summary planes), 55,888 B and 15,392 B (32 x 32 level planes and split, four
levels)."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "gp_dla_detection_amd" / "csrc"
GRIDS = [(1, 1), (7, 5), (12, 27), (32, 32)]

PROGRAM = r"""
#include <cstdio>
#include "row_posterior.h"
using namespace gpdla;
int main() {
  const int grids[4][2] = {{1, 1}, {7, 5}, {12, 27}, {32, 32}};
  for (auto& g : grids) {
    const int nz = g[0], nn = g[1];
    std::printf("summary %d %d 0 %zu\n", nz, nn, planes_lds(nz, nn, kRowTileOne, 1, true).total);
    std::printf("summary_map %d %d 0 %zu\n", nz, nn, planes_lds(nz, nn, kRowTileOne, 1, false).total);
    std::printf("pop %d %d 0 %zu\n", nz, nn, split_lds(nz, nn, kRowTileOne, 1, 1).total);
    for (int lv = 1; lv <= kMaxDlas; ++lv) {
      std::printf("level_planes %d %d %d %zu\n", nz, nn, lv, planes_lds(nz, nn, kRowTileLevels, lv).total);
      std::printf("level_split %d %d %d %zu\n", nz, nn, lv, split_lds(nz, nn, kRowTileLevels, lv, kMaxDlas).total);
    }
  }
  return 0;
}
"""


def up16(x):
    return (x + 15) & ~15


def carve(sizes):
    o = 0
    for s in sizes:
        o = up16(o + s)
    return o


# the four carves as the kernels laid them out by hand: 4 waves, 5 planes, tiles of 512 (level 1) and 256 samples,
# 16 candidate slots, kMaxDlas = 4
def summary_lds(nz, nn, planes):
    grid = [(nz + 1) * 8, (nn + 1) * 8, 5 * nz * nn * 8, 512 * 8, 512 * 8, 512 * 4] if planes else []
    return carve([4 * 8, 4 * 4] + grid)


def pop_lds(nz, nn):
    return carve([4 * 8, 4 * 4, (nz + 1) * 8, (nn + 1) * 8, nz * nn * 8, 512 * 8, 512 * 4, 16 * 8, 16 * 4, 16 * 4, 4])


def level_planes_lds(nz, nn, levels):
    return carve([4 * 8, 4 * 4, (nz + 1) * 8, (nn + 1) * 8, 5 * nz * nn * 8, 256 * 8, 256 * levels * 8, 256 * levels * 4])


def level_split_lds(nz, nn, levels):
    return carve([4 * 8, 4 * 4, (nz + 1) * 8, (nn + 1) * 8, nz * nn * 8, 256 * 8, 256 * levels * 4, 16 * 8, 16 * 4,
                  16 * 4 * 4, 4])


def test_carve_totals_are_the_hand_laid_ones(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = tmp_path / "row_lds.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "row_lds"
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O0", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        kind, nz, nn, lv, total = line.split()
        got[(kind, int(nz), int(nn), int(lv))] = int(total)
    assert len(got) == len(GRIDS) * (3 + 2 * 4)
    for nz, nn in GRIDS:
        assert got[("summary", nz, nn, 0)] == summary_lds(nz, nn, True)
        assert got[("summary_map", nz, nn, 0)] == summary_lds(nz, nn, False) == 48
        assert got[("pop", nz, nn, 0)] == pop_lds(nz, nn)
        for lv in (1, 2, 3, 4):
            assert got[("level_planes", nz, nn, lv)] == level_planes_lds(nz, nn, lv), (nz, nn, lv)
            assert got[("level_split", nz, nn, lv)] == level_split_lds(nz, nn, lv), (nz, nn, lv)
    assert got[("summary", 32, 32, 0)] == 51792
    assert got[("level_planes", 32, 32, 4)] == 55888
    assert got[("level_split", 32, 32, 4)] == 15392

"""gmr_amd/csrc/target_blocks.h without a GPU: a stand-alone C++ program (its own main, built with the host compiler under
AddressSanitizer and UBSan, never loaded into Python) walks a run of frames the way the IK kernel's frame loop does and checks which
lane prepares which (frame, slot) into which ring image, for nslot 1..16 and every (kf0, kend) of up to 12 frames."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gmr_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "target_blocks.h"

using namespace gmr;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s (nslot %d kf0 %d kend %d kf %d)\n", __LINE__, #c, nslot, kf0, kend, kf); exit(1); } } while (0)

int main() {
  static_assert(kTargetBlockFrames * kTargetBlockLanes == 64, "a block fills one wavefront");
  long blocks = 0;
  for (int nslot = 1; nslot <= kTargetBlockLanes; ++nslot)
    for (int kf0 = 0; kf0 <= 12; ++kf0)
      for (int kend = kf0; kend <= kf0 + 12; ++kend) {
        // ring[image][slot]: the frame whose targets the image holds, -1 = never written
        std::vector<int> ring(kTargetBlockFrames * kTargetBlockLanes, -1);
        for (int kf = kf0; kf < kend; ++kf) {  // the kernel's frame loop
          if (target_block_starts(kf0, kf)) {
            ++blocks;
            CHECK((kf - kf0) % kTargetBlockFrames == 0);
            const int last = kf + kTargetBlockFrames - 1 < kend - 1 ? kf + kTargetBlockFrames - 1 : kend - 1;
            std::vector<int> seen((last - kf + 1) * nslot, 0);
            for (int lane = 0; lane < 64; ++lane) {
              const TargetBlockLane t = target_block_lane(lane, nslot, kf, kend);
              CHECK(t.image >= 0 && t.image < kTargetBlockFrames && t.slot >= 0 && t.slot < kTargetBlockLanes);
              CHECK(t.image == target_block_image(kf0, t.frame));
              if (!t.on) {  // no frame at or beyond kend, no slot the model lacks
                CHECK(t.slot >= nslot || t.frame >= kend);
                continue;
              }
              CHECK(t.slot < nslot);
              CHECK(t.frame >= kf && t.frame <= last && t.frame < kend);  // in range
              CHECK(seen[(t.frame - kf) * nslot + t.slot]++ == 0);          // every enabled lane a distinct (frame, slot)
              ring[t.image * kTargetBlockLanes + t.slot] = t.frame;
            }
            for (int v : seen) CHECK(v == 1);  // every frame of the block covered for every slot
          } else {
            CHECK((kf - kf0) % kTargetBlockFrames != 0);
          }
          // what frame kf reads was prepared for frame kf, in every slot, and not overwritten by a later block
          const int img = target_block_image(kf0, kf);
          CHECK(img >= 0 && img < kTargetBlockFrames);
          for (int s = 0; s < nslot; ++s) CHECK(ring[img * kTargetBlockLanes + s] == kf);
        }
      }
  printf("ok %ld\n", blocks);
  return 0;
}
"""


def test_target_block_mapping_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    src, exe = tmp_path / "target_blocks_test.cpp", tmp_path / "target_blocks_test"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert int(r.stdout.split()[1]) > 1000


def test_target_blocks_header_is_plain_cxx():
    """No HIP include: the stand-alone build above and the kernel share the header."""
    text = open(os.path.join(CSRC, "target_blocks.h")).read()
    assert "hip" not in "\n".join(ln for ln in text.split("\n") if ln.lstrip().startswith("#include"))

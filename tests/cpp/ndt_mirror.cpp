// Drives pcgx::NDTMap and pcgx::NDT (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_ndt.py
// compares with the Python binding's results.
// Input: a text file written by the test
//   G res sx sy sz ox oy oz    the grid
//   B n   followed by n lines "x y z"   the base cloud (grid and map are built over it)
//   T n   followed by n lines "x y z"   the target
//   F neighbors max_iteration           run Evaluate (identity) and Fit
// Output: "C occupied valid", one line "V addr count valid" per voxel, "S" + 30 sums (%.17g), "P" + 16 pose floats
// (%.9g) + the number of iterations.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    float res = 1.0f;
    std::array<int64_t, 3> size{1, 1, 1};
    pcgx::Vec3 origin{0, 0, 0};
    std::vector<pcgx::Vec3> base, target;
    while (in >> tag) {
      if (tag == "G") {
        in >> res >> size[0] >> size[1] >> size[2] >> origin[0] >> origin[1] >> origin[2];
      } else if (tag == "B" || tag == "T") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> &pts = tag == "B" ? base : target;
        pts.resize(n);
        for (auto &p : pts) in >> p[0] >> p[1] >> p[2];
      } else if (tag == "F") {
        int32_t nb, iters;
        in >> nb >> iters;
        const pcgx::CloudView cv{base.data(), (int64_t)base.size(), 12, 0};
        pcgx::BucketVoxelGrid vg(res, size, origin, cv);
        pcgx::NDTMap map(vg, cv);
        std::printf("C %" PRId64 " %" PRId64 "\n", map.Occupied(), map.Valid());
        const auto cells = map.Cells();
        for (size_t i = 0; i < cells.addr.size(); i++)
          std::printf("V %" PRId64 " %d %d\n", cells.addr[i], (int)cells.count[i], (int)cells.valid[i]);
        const auto s = map.Evaluate(target, nullptr, nb);
        std::printf("S");
        for (double v : s) std::printf(" %.17g", v);
        std::printf("\n");
        pcgx::NDT ndt;
        ndt.Neighbors = nb;
        ndt.MaxIteration = iters;
        ndt.Threshold.fill(-1.0f);
        const auto fit = ndt.Fit(map, target);
        std::printf("P");
        for (float v : fit.first) std::printf(" %.9g", v);
        std::printf(" %d\n", fit.second.NumIteration);
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}

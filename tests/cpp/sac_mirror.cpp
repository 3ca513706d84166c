// Drives the C++ mirror of pc/sac (pcgol_amd/host/pcgx.hpp, pcgx::sac) over the C ABI and prints what
// tests/test_cpp_sac.py compares with the reference's tables (tests/golden/ref_sac.json) and the oracle.
// Input: a text file written by the test
//   G res sx sy sz ox oy oz n   followed by n lines "x y z"   grid + cloud (Add(p, i) for every point)
//   F a b c d                   Fit([a, b, c]); Inliers(d) sorted; IsIn of every point with d
//   S seed n d                  SAC with a seeded RandomSampler, Compute(n), Inliers(d) of Coefficients()
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <memory>
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
    std::vector<pcgx::Vec3> pts;
    std::unique_ptr<pcgx::BucketVoxelGrid> grid;
    std::unique_ptr<pcgx::sac::VoxelGridSurfaceModel> model;
    while (in >> tag) {
      if (tag == "G") {
        float res;
        std::array<int64_t, 3> size;
        pcgx::Vec3 origin;
        size_t n;
        in >> res >> size[0] >> size[1] >> size[2] >> origin[0] >> origin[1] >> origin[2] >> n;
        pts.resize(n);
        for (auto &p : pts) in >> p[0] >> p[1] >> p[2];
        const pcgx::CloudView cv{pts.data(), (int64_t)pts.size(), 12, 0};
        model.reset();
        grid.reset(new pcgx::BucketVoxelGrid(res, size, origin, cv));
        model.reset(new pcgx::sac::VoxelGridSurfaceModel(*grid, cv));
      } else if (tag == "F") {
        int64_t a, b, c;
        float d;
        in >> a >> b >> c >> d;
        auto co = model->Fit({a, b, c});
        if (!co) {
          std::printf("fit %" PRId64 " %" PRId64 " %" PRId64 " failed\n", a, b, c);
          continue;
        }
        std::printf("fit %" PRId64 " %" PRId64 " %" PRId64 " ok score %" PRId64 " inliers", a, b, c, co->Evaluate());
        for (int64_t i : co->Inliers(d)) std::printf(" %" PRId64, i);
        std::printf(" isin ");
        for (const auto &p : pts) std::printf("%d", co->IsIn(p, d) ? 1 : 0);
        std::printf("\n");
      } else if (tag == "S") {
        uint64_t seed;
        int n;
        float d;
        in >> seed >> n >> d;
        pcgx::sac::RandomSampler smp((int64_t)pts.size(), seed);
        pcgx::sac::SAC s(smp, *model);
        const bool found = s.Compute(n);
        std::printf("sac %d", found ? 1 : 0);
        if (found) {
          std::printf(" score %" PRId64 " inliers", s.Coefficients()->Evaluate());
          for (int64_t i : s.Coefficients()->Inliers(d)) std::printf(" %" PRId64, i);
        }
        std::printf("\n");
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}

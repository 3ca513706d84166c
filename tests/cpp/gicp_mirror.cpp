// Drives pcgx::GeneralizedICP (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_gicp.py
// compares with the Python binding's results.
// Input: a text file written by the test
//   B n            followed by n lines "x y z"   the base cloud (a tree over it)
//   T m            followed by m lines "x y z"   the target
//   F k eps max_dist iters                       Covariances(k, inf, PLANE, eps) of both clouds, then Fit, then FitKNN
// Output: two lines (Fit, FitKNN) "num_iteration num_pairs value t0 .. t15 h0 .. h35" (%.9g: float32 round trips exactly).
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

static void print(const std::pair<pcgx::Mat4, pcgx::PlaneStat> &r) {
  std::printf("%d %lld %.9g", r.second.NumIteration, (long long)r.second.Evaluated.num_pairs, r.second.Evaluated.value);
  for (float v : r.first) std::printf(" %.9g", v);
  for (float v : r.second.Hessian) std::printf(" %.9g", v);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    std::vector<pcgx::Vec3> base, target;
    while (in >> tag) {
      if (tag == "B" || tag == "T") {
        size_t n;
        in >> n;
        std::vector<pcgx::Vec3> &pts = tag == "B" ? base : target;
        pts.resize(n);
        for (auto &p : pts) in >> p[0] >> p[1] >> p[2];
      } else if (tag == "F") {
        int32_t k, iters;
        float eps, max_dist;
        in >> k >> eps >> max_dist >> iters;
        pcgx::KDTree bt(base), tt(target);
        pcgx::GeneralizedICP reg;
        reg.MaxDist = max_dist;
        reg.MinPairs = 6;
        reg.Threshold.fill(-1.0f);
        reg.MaxIteration = iters;
        print(reg.Fit(bt, bt.Covariances(k, std::numeric_limits<float>::infinity(), PCGX_COV_PLANE, eps).cov, target,
                      tt.Covariances(k, std::numeric_limits<float>::infinity(), PCGX_COV_PLANE, eps).cov));
        print(reg.FitKNN(bt, target, k, eps));
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}

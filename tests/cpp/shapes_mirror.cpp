// Drives pcgx::KDTree::Shapes (pcgol_amd/host/pcgx.hpp) over the C ABI and prints what tests/test_cpp_shapes.py compares
// with the Python binding's results.
// Input: a text file written by the test
//   P n                              followed by n lines "x y z mx my mz": the cloud (a tree over it) and its normals
//   W k                              followed by k random words: the samples of the calls that follow
//   C kind maxDist nHyp maxShapes minInliers sampleRadius rMin rMax hasAxis ax ay az minAxisCos minNormalCos refine
// Output per C: "L label ..." (one per point), "S size ..." (one per shape), "I id ..." (the inliers, shape by shape),
// "B best ..." and "R refined ..." (one per shape), "T status ..." and "N count ..." (one per round and hypothesis),
// "F bits ..." (the shapes as float32 bit patterns), "H bits ..." (the hypotheses' records), "M id ..." (Members of the
// last shape).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../pcgol_amd/host/pcgx.hpp"

static void line(const char *tag, const std::vector<int64_t> &v) {
  std::printf("%s", tag);
  for (int64_t x : v) std::printf(" %" PRId64, x);
  std::printf("\n");
}

static std::vector<int64_t> bits(const std::vector<float> &v) {
  std::vector<int64_t> out(v.size());
  for (size_t k = 0; k < v.size(); k++) {
    uint32_t b;
    std::memcpy(&b, &v[k], 4);
    out[k] = b;
  }
  return out;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    pcgx::check(pcgx_init(0));
    pcgx::CheckAbi();
    std::ifstream in(argv[1]);
    std::string tag;
    std::unique_ptr<pcgx::KDTree> tree;
    std::vector<pcgx::Vec3> pts, nrm;
    std::vector<uint32_t> words;
    while (in >> tag) {
      if (tag == "P") {
        size_t n;
        in >> n;
        pts.resize(n);
        nrm.resize(n);
        for (size_t i = 0; i < n; i++) in >> pts[i][0] >> pts[i][1] >> pts[i][2] >> nrm[i][0] >> nrm[i][1] >> nrm[i][2];
        tree.reset(new pcgx::KDTree(pts));
      } else if (tag == "W") {
        size_t k;
        in >> k;
        words.resize(k);
        for (size_t i = 0; i < k; i++) in >> words[i];
      } else if (tag == "C") {
        float max_dist, sample_radius, r_min, r_max, axis[3], min_axis_cos, min_normal_cos;
        int64_t n_hyp, min_inliers;
        int kind, max_shapes, has_axis, refine;
        in >> kind >> max_dist >> n_hyp >> max_shapes >> min_inliers >> sample_radius >> r_min >> r_max >> has_axis >>
            axis[0] >> axis[1] >> axis[2] >> min_axis_cos >> min_normal_cos >> refine;
        const std::vector<uint32_t> smp(words.begin(), words.begin() + (std::ptrdiff_t)(2 * n_hyp * max_shapes));
        const auto res = tree->Shapes(kind, max_dist, nrm, smp, n_hyp, max_shapes, min_inliers, sample_radius, r_min, r_max,
                                      has_axis ? axis : nullptr, min_axis_cos, min_normal_cos, refine != 0);
        line("L", res.labels);
        line("S", res.sizes);
        line("I", res.ids);
        line("B", res.best);
        line("R", std::vector<int64_t>(res.refined.begin(), res.refined.end()));
        line("T", std::vector<int64_t>(res.status.begin(), res.status.end()));
        line("N", res.counts);
        line("F", bits(res.shapes));
        line("H", bits(res.hypShapes));
        line("M", res.sizes.empty() ? std::vector<int64_t>() : res.Members(res.sizes.size() - 1));
      }
    }
  } catch (const pcgx::Error &e) {
    std::fprintf(stderr, "pcgx error %d: %s\n", (int)e.code, e.what());
    return 1;
  }
  return 0;
}

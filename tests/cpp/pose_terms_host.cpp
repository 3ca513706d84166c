// csrc/pose_terms.h on the host (tests/test_pose_terms_host.py): the expressions the kernels compile, as a stand-alone
// program over a binary file the test writes.
//   in:  int64 ns, nd, m, n_hyp, n_refit;  float32 edge_similarity;  float32 src[3 ns], dst[3 nd];  int32 src_ids[m],
//        dst_ids[m];  uint32 samples[3 n_hyp];  int32 refit_ids[n_refit] (pairs, ascending)
//   out: int32 status[n_hyp];  float32 poses[16 n_hyp];  then, with n_refit > 0: int32 allowed;  float32 pose[16];
//        float64 l1, l2  -- the refit over refit_ids, its moments about the first pair's points
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "pose_terms.h"

using namespace pcgx;

template <class T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hd[5];
  float es;
  if (fread(hd, 8, 5, f) != 5 || fread(&es, 4, 1, f) != 1) return 3;
  const int64_t ns = hd[0], nd = hd[1], m = hd[2], n_hyp = hd[3], n_refit = hd[4];
  std::vector<float> src, dst;
  std::vector<int32_t> si, di, ri;
  std::vector<uint32_t> sm;
  if (!rd(f, src, (size_t)ns * 3) || !rd(f, dst, (size_t)nd * 3) || !rd(f, si, (size_t)m) || !rd(f, di, (size_t)m) ||
      !rd(f, sm, (size_t)n_hyp * 3) || !rd(f, ri, (size_t)n_refit))
    return 3;
  fclose(f);
  std::vector<int32_t> status((size_t)n_hyp);
  std::vector<float> poses((size_t)n_hyp * 16);
  for (int64_t h = 0; h < n_hyp; h++)
    status[(size_t)h] = pose_hypothesis(src.data(), ns, dst.data(), nd, si.data(), di.data(), m, &sm[(size_t)h * 3], es,
                                        &poses[(size_t)h * 16]);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(status.data(), 4, status.size(), o);
  fwrite(poses.data(), 4, poses.size(), o);
  if (n_refit > 0) {
    const float *op = &src[(size_t)si[(size_t)ri[0]] * 3], *oq = &dst[(size_t)di[(size_t)ri[0]] * 3];
    PoseMoments a;
    pose_moments_clear(a);
    for (int64_t i = 0; i < n_refit; i++)
      pose_moments_add(a, &src[(size_t)si[(size_t)ri[(size_t)i]] * 3], &dst[(size_t)di[(size_t)ri[(size_t)i]] * 3], op, oq);
    float pose[16];
    double l[2];
    const bool solved = pose_solve(a, op, oq, pose, l[0], l[1]);
    const int32_t allowed = pose_refit_allowed(a.n, solved, l[0], l[1]) ? 1 : 0;
    fwrite(&allowed, 4, 1, o);
    fwrite(pose, 4, 16, o);
    fwrite(l, 8, 2, o);
  }
  fclose(o);
  return 0;
}

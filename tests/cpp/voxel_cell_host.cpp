// csrc/voxel_cell.h on the host (tests/test_voxel_cell_host.py): a program of its own, built with
// -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all, so that a conversion or an index sum the C++
// standard leaves undefined ends it instead of "happening to work".  The header compiles over tests/cpp/host_shim.
//
// stdin, one case after the other, every float as the hexadecimal word of its bits:
//   leaf[3] chunk[3] (decimal) mm6[6] npts, then npts lines of x y z
// stdout per case: "grid <status> <chunked> <xs> <ys> <n_voxels> <nx> <ny> <n_chunks>", then -- only where status is 0,
// as on the device -- per point "<bad> <cid> <cell> <bad> <cid> <cell>": voxel_key_xyz (the 32-bit lanes first) and
// voxel_key_xyz_any (the general form), which have to agree.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "voxel_cell.h"

using namespace pcgx;

static bool read_f32(float *f) {
  unsigned int w;
  if (scanf("%x", &w) != 1) return false;
  const uint32_t bits = w;
  memcpy(f, &bits, 4);
  return true;
}

int main() {
  for (;;) {
    float leaf[3], mm6[6];
    int32_t chunk[3];
    long long npts;
    if (!read_f32(&leaf[0])) return 0;  // end of input
    if (!read_f32(&leaf[1]) || !read_f32(&leaf[2])) return 2;
    if (scanf("%d %d %d", &chunk[0], &chunk[1], &chunk[2]) != 3) return 2;
    for (int k = 0; k < 6; k++)
      if (!read_f32(&mm6[k])) return 2;
    if (scanf("%lld", &npts) != 1 || npts < 0) return 2;
    std::vector<float> pts((size_t)npts * 3);
    for (float &v : pts)
      if (!read_f32(&v)) return 2;
    VoxelParams vp;
    const int status = voxel_grid_params(mm6, leaf, chunk, vp);
    printf("grid %d %d %lld %lld %lld %lld %lld %lld\n", status, (int)vp.chunked, (long long)vp.xs, (long long)vp.ys,
           (long long)vp.n_voxels, (long long)vp.nx, (long long)vp.ny, (long long)vp.n_chunks);
    if (status != 0) continue;
    for (long long i = 0; i < npts; i++) {
      uint32_t cid = 0, ka = 0, cid_any = 0, ka_any = 0;
      bool bad = false, bad_any = false;
      voxel_key_xyz(&pts[(size_t)i * 3], vp, cid, ka, bad);
      voxel_key_xyz_any(&pts[(size_t)i * 3], vp, cid_any, ka_any, bad_any);
      printf("%d %u %u %d %u %u\n", bad ? 1 : 0, cid, ka, bad_any ? 1 : 0, cid_any, ka_any);
    }
  }
}

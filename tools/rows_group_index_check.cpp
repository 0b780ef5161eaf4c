// Host check of the index arithmetic of dec_gemm_rows' row groups: the grid of a launch, the group offsets of a / r / y /
// x_out, the row count of the last group and the staging / epilogue thread maps are the expressions of
// csrc/s1_decode_rows_index.h, which the kernel (csrc/s1_decode_rows.hip) is written with; here they are replayed thread
// by thread on exactly sized heap arrays.  Built with a host compiler and -fsanitize=address,undefined, an access outside
// a buffer stops the run; the program itself checks that every element of y is written exactly once, x_out once per row
// (by the blockIdx.x == 0 block of the row's group) and nothing else.  No GPU is involved.
// tests/test_s1_rows_index_cpu.py builds and runs it (without the sanitizers, row counts next to a tile or group boundary:
// argument "edges") with every suite run.
//   c++ -O1 -g -fsanitize=address,undefined tools/rows_group_index_check.cpp -o rows_group_index_check && ./rows_group_index_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../easevoice_trainer_amd/csrc/s1_decode_rows_index.h"

namespace {
using namespace evt_rows;

struct Launch {
  int B, N, K;
  std::vector<float> a, r;
  std::vector<int> y, x_out;      // write counts
};

void block(Launch& L, int bx, int by, bool ln) {
  const int K = L.K, N = L.N, NCH = K / kKC;
  const int n0 = bx * 16;
  const int g0 = group_first(by);
  const int B = group_rows(L.B, g0);
  if (B < 1 || B > kRows) { std::printf("group of %d rows (B=%d, group %d)\n", B, L.B, by); std::exit(1); }
  const float* a = L.a.data() + row_offset(g0, K);
  const float* r = L.r.data() + row_offset(g0, K);
  int* x_out = L.x_out.data() + row_offset(g0, K);
  int* y = L.y.data() + row_offset(g0, N);
  const int nbt = b_tiles(B), rows_used = nbt * 16;
  volatile float sink = 0.f;
  for (int tid = 0; tid < kThreads; ++tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int k4 = stage_k4(tid), rb = stage_row0(tid);
    for (int c = 0; c < NCH; ++c)
      for (int i = 0; i < kXPT; ++i) {
        const int b = rb + 4 * i;
        if (b < B) {        // load_chunk
          const long o = stage_offset(b, K, c, k4);
          for (int e = 0; e < 4; ++e) sink = sink + a[o + e] + (ln ? r[o + e] : 0.f);
        }
        if (b >= rows_used) continue;      // store_chunk
        if (ln && b < B && bx == 0)
          for (int e = 0; e < 4; ++e) ++x_out[stage_offset(b, K, c, k4) + e];
      }
    if (ln)
      for (int b = wave; b < B; b += kNW)
        for (int k = lane * 4; k < K; k += 256)
          for (int e = 0; e < 4; ++e) sink = sink + a[(long)b * K + k + e] + r[(long)b * K + k + e];
    const int eb = epi_row(tid), en = epi_col(tid);
    if (eb < B && n0 + en < N) ++y[(long)eb * N + n0 + en];
  }
}
}  // namespace

int main(int argc, char** argv) {
  // "edges": only the row counts next to a b-tile or a group boundary (what the test suite runs); default: every B
  const bool edges = argc > 1 && std::string(argv[1]) == "edges";
  long launches = 0;
  for (int N : {512, 1025, 1536, 2048})
    for (int K : {512, 2048}) {
      if (K == 2048 && N != 512) continue;      // the layer shapes: K = 2048 belongs to ffn2 (N = 512)
      for (int B = 1; B <= kRowsMax; ++B)
        for (int ln = 0; ln < 2; ++ln) {
          if (edges && B % 16 > 1 && B % 16 < 15 && B != 100) continue;
          Launch L{B, N, K, std::vector<float>((size_t)B * K, 1.f), std::vector<float>((size_t)B * K, 1.f),
                   std::vector<int>((size_t)B * N, 0), std::vector<int>((size_t)B * K, 0)};
          const int gx = grid_x(N), gy = grid_y(B);
          if (gy < 1 || gy > kRowsMax / kRows || (B <= kRows && gy != 1)) { std::printf("grid y %d for B=%d\n", gy, B); return 1; }
          for (int by = 0; by < gy; ++by)
            for (int bx = 0; bx < gx; ++bx) block(L, bx, by, ln != 0);
          for (int v : L.y)
            if (v != 1) { std::printf("y written %d times (B=%d N=%d K=%d)\n", v, B, N, K); return 1; }
          for (int v : L.x_out)
            if (v != ln) { std::printf("x_out written %d times (B=%d N=%d K=%d ln=%d)\n", v, B, N, K, ln); return 1; }
          ++launches;
        }
    }
  std::printf("ok: %ld launches replayed, B within 1..%d, every y element written once, x_out once per row\n", launches, kRowsMax);
  return 0;
}

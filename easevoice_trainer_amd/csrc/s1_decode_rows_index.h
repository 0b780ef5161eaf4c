// Row-group index arithmetic of dec_gemm_rows (s1_decode_rows.hip), shared with the host replay
// tools/rows_group_index_check.cpp, which runs exactly these expressions on exactly sized heap arrays under a sanitizer.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define EVT_ROWS_HD __host__ __device__
#else
#define EVT_ROWS_HD
#endif

namespace evt_rows {
constexpr int kRows = 32;            // batch rows per workgroup (one row group): two 16-column MFMA tiles
constexpr int kRowsMax = 128;        // batch rows per launch: up to four row groups on blockIdx.y
constexpr int kNW = 8;               // waves per workgroup
constexpr int kThreads = kNW * 64;
constexpr int kKC = 512;             // K chunk staged in LDS
constexpr int kXPT = kRows * kKC / 4 / kThreads;   // float4 of one chunk of x per thread while staging (8)

EVT_ROWS_HD inline int grid_x(int N) { return (N + 15) / 16; }                   // 16-row tiles of W
EVT_ROWS_HD inline int grid_y(int B) { return (B + kRows - 1) / kRows; }         // row groups
EVT_ROWS_HD inline int group_first(int by) { return by * kRows; }                // first batch row of group `by`
EVT_ROWS_HD inline int group_rows(int B, int g0) { return B - g0 < kRows ? B - g0 : kRows; }   // 1..32, the last may be short
EVT_ROWS_HD inline int b_tiles(int Bg) { return (Bg + 15) >> 4; }                // b-tiles in use (1 or 2)
EVT_ROWS_HD inline long row_offset(int g0, int width) { return (long)g0 * width; }             // of a / r / x_out (K), y (N)
// staging: thread -> columns 4*k4 .. 4*k4+3 of rows stage_row0 + 4*i, i < kXPT
EVT_ROWS_HD inline int stage_k4(int tid) { return tid & (kKC / 4 - 1); }
EVT_ROWS_HD inline int stage_row0(int tid) { return tid >> 7; }
EVT_ROWS_HD inline long stage_offset(int b, int K, int c, int k4) { return (long)b * K + c * kKC + 4 * k4; }
// epilogue: thread -> batch row tid >> 4, weight row tid & 15 of the tile
EVT_ROWS_HD inline int epi_row(int tid) { return tid >> 4; }
EVT_ROWS_HD inline int epi_col(int tid) { return tid & 15; }
}  // namespace evt_rows

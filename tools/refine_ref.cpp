// refine_ref -- single-thread C++ restatement of the point refiner (include/picp_c.h
// picp_refine_*), in double and in the operation order of the numpy oracle
// (tests/refine_oracle.py): the CPU figure tools/refine_bench.py prints beside the kernel's, and
// checked against that oracle by tests/test_refine_cpu.py.
//
//   refine_ref problem.bin result.bin [reps]
//
// problem.bin (tools/refine_bench.py write_problem): int64 n_poses n_points n_obs rows cols;
// float K[9] row-major; float threshold damping; int32 min_inliers keep_outliers max_rounds; float
// conv_eps; float poses[16 n_poses] row-major world-in-camera; int64 off[n_points + 1]; int32
// obs_pose[n_obs]; float obs_uv[2 n_obs]; float xyz[3 n_points].
// result.bin: double xyz[3 n_points]; int32 (n_in n_projected rounds ok converged)[n_points].
// Prints one JSON line: the best wall time of reps runs (every run starts from the file's points).
#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Problem {
  int64_t n_poses, n_points, n_obs, rows, cols;
  float K[9], threshold, damping;
  int32_t min_inliers, keep_outliers, max_rounds;
  float conv_eps;
  std::vector<float> poses, uv, xyz;
  std::vector<int64_t> off;
  std::vector<int32_t> obs_pose;
};

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

static bool load(const char* path, Problem& P) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int64_t hdr[5];
  bool ok = rd(f, hdr, 5);
  P.n_poses = hdr[0]; P.n_points = hdr[1]; P.n_obs = hdr[2]; P.rows = hdr[3]; P.cols = hdr[4];
  ok = ok && P.n_poses >= 0 && P.n_points >= 0 && P.n_obs >= 0;
  ok = ok && rd(f, P.K, 9) && rd(f, &P.threshold, 1) && rd(f, &P.damping, 1) && rd(f, &P.min_inliers, 1) &&
       rd(f, &P.keep_outliers, 1) && rd(f, &P.max_rounds, 1) && rd(f, &P.conv_eps, 1);
  if (ok) {
    P.poses.resize(16 * P.n_poses);
    P.off.resize(P.n_points + 1);
    P.obs_pose.resize(P.n_obs);
    P.uv.resize(2 * P.n_obs);
    P.xyz.resize(3 * P.n_points);
    ok = rd(f, P.poses.data(), P.poses.size()) && rd(f, P.off.data(), P.off.size()) &&
         rd(f, P.obs_pose.data(), P.obs_pose.size()) && rd(f, P.uv.data(), P.uv.size()) &&
         rd(f, P.xyz.data(), P.xyz.size());
  }
  fclose(f);
  if (!ok) return false;
  if (P.off[0] != 0 || P.off[P.n_points] != P.n_obs) return false;
  for (int64_t i = 0; i < P.n_points; ++i)
    if (P.off[i + 1] < P.off[i]) return false;
  for (int64_t k = 0; k < P.n_obs; ++k)
    if (P.obs_pose[k] < 0 || P.obs_pose[k] >= P.n_poses) return false;
  return true;
}

static void refine(const Problem& P, std::vector<double>& X, std::vector<int32_t>& st) {
  const double thr = P.threshold, damping = P.damping, eps = P.conv_eps;
  const double maxx = (double)(P.cols - 1), maxy = (double)(P.rows - 1);
  double K[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K[r][c] = P.K[3 * r + c];
  for (int64_t i = 0; i < P.n_points; ++i) {
    double x[3] = {P.xyz[3 * i], P.xyz[3 * i + 1], P.xyz[3 * i + 2]};
    double prev = FLT_MAX;
    int32_t s_in = 0, s_proj = 0, rounds = 0, okf = 0, conv = 0;
    for (int round = 0; round < P.max_rounds; ++round) {
      double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, chi_in = 0;
      int32_t n_in = 0, n_proj = 0;
      for (int64_t o = P.off[i]; o < P.off[i + 1]; ++o) {
        const float* T = &P.poses[16 * (size_t)P.obs_pose[o]];  // row-major 4x4
        double pc[3], ph[3];
        for (int r = 0; r < 3; ++r) pc[r] = ((T[4 * r] * x[0] + T[4 * r + 1] * x[1]) + T[4 * r + 2] * x[2]) + T[4 * r + 3];
        for (int r = 0; r < 3; ++r) ph[r] = (K[r][0] * pc[0] + K[r][1] * pc[1]) + K[r][2] * pc[2];
        const double iz = 1.0 / ph[2], ix = ph[0] * iz, iy = ph[1] * iz;
        if (pc[2] <= 0 || ix < 0 || ix > maxx || iy < 0 || iy > maxy) continue;
        ++n_proj;
        const double e0 = ix - P.uv[2 * o], e1 = iy - P.uv[2 * o + 1];
        const double chi = e0 * e0 + e1 * e1;
        double lam = 1.0;
        if (chi > thr) {
          lam = std::sqrt(thr / chi);
          if (!P.keep_outliers) continue;
        } else {
          chi_in += chi;
          ++n_in;
        }
        const double iz2 = iz * iz, jp0 = -(ph[0] * iz2), jp1 = -(ph[1] * iz2);
        double J[2][3];
        for (int c = 0; c < 3; ++c) {
          const double a0[3] = {iz * K[0][0] + jp0 * K[2][0], iz * K[0][1] + jp0 * K[2][1], iz * K[0][2] + jp0 * K[2][2]};
          const double a1[3] = {iz * K[1][0] + jp1 * K[2][0], iz * K[1][1] + jp1 * K[2][1], iz * K[1][2] + jp1 * K[2][2]};
          J[0][c] = (a0[0] * T[c] + a0[1] * T[4 + c]) + a0[2] * T[8 + c];
          J[1][c] = (a1[0] * T[c] + a1[1] * T[4 + c]) + a1[2] * T[8 + c];
        }
        int k = 0;
        for (int a = 0; a < 3; ++a) {
          for (int c = a; c < 3; ++c) H[k++] += (lam * J[0][a]) * J[0][c] + (lam * J[1][a]) * J[1][c];
          b[a] += (lam * J[0][a]) * e0 + (lam * J[1][a]) * e1;
        }
      }
      s_in = n_in;
      s_proj = n_proj;
      if (n_in < P.min_inliers) {
        okf = 0;
        break;
      }
      const double d0 = H[0] + damping, h11 = H[3] + damping, h22 = H[5] + damping;
      const double i0 = 1.0 / d0, l10 = H[1] * i0, l20 = H[2] * i0;
      const double d1 = h11 - l10 * H[1], i1 = 1.0 / d1;
      const double l21 = (H[4] - l20 * H[1]) * i1;
      const double d2 = h22 - l20 * H[2] - l21 * (l21 * d1), i2 = 1.0 / d2;
      const double y0 = -b[0], y1 = -b[1] - l10 * y0, y2 = -b[2] - l20 * y0 - l21 * y1;
      const double x2 = y2 * i2, x1 = y1 * i1 - l21 * x2, x0 = y0 * i0 - l10 * x1 - l20 * x2;
      if (!(d0 > 0 && d1 > 0 && d2 > 0 && std::isfinite(x0) && std::isfinite(x1) && std::isfinite(x2))) {
        okf = 0;
        break;
      }
      x[0] += x0;
      x[1] += x1;
      x[2] += x2;
      okf = 1;
      ++rounds;
      const double rel = (prev > 1e-10) ? std::fabs(prev - chi_in) / prev : 0.0;
      if (rel < eps) {
        conv = 1;
        break;
      }
      prev = chi_in;
    }
    for (int c = 0; c < 3; ++c) X[3 * i + c] = x[c];
    int32_t* s = &st[5 * i];
    s[0] = s_in; s[1] = s_proj; s[2] = rounds; s[3] = okf; s[4] = conv;
  }
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: refine_ref problem.bin result.bin [reps]\n");
    return 2;
  }
  Problem P;
  if (!load(argv[1], P)) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  const int reps = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
  std::vector<double> X(3 * P.n_points);
  std::vector<int32_t> st(5 * P.n_points);
  double best = 1e300;
  for (int r = 0; r < reps; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    refine(P, X, st);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    best = std::min(best, us);
  }
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(X.data(), sizeof(double), X.size(), f) != X.size() ||
      fwrite(st.data(), sizeof(int32_t), st.size(), f) != st.size()) {
    fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  fclose(f);
  printf("{\"cpu_us\": %.1f, \"n_points\": %lld, \"n_obs\": %lld}\n", best, (long long)P.n_points, (long long)P.n_obs);
  return 0;
}

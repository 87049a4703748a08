// dgs::HipOdometryFleet (include/dgs/odometry_fleet_hip.hpp) against the Eigen stub (tests/stub_pcl): B scan-matching odometry streams advanced
// frame by frame, every step one device call chain.
//   odometry_fleet_driver <FAST_GICP|GICP_HIP> in.bin out.bin <batch_independent 0|1> <max_correspondence_distance> <leaf_size> <transformation_epsilon>
// in.bin: int64 B; per stream 6 doubles (keyframe_delta_trans, _angle, _time, transform_thresholding, max_acceptable_trans, _angle); int64 F;
//         per frame, per stream: int64 n (-1: the stream has no frame), double stamp, n x 4 floats.
// out.bin: per frame, per stream: 16 floats odom and 16 floats relative pose (column-major), int32 converged, int32 keyframes, double
//          matching_error, double inlier_fraction (status fields of a stream that was not registered in the frame: zeros).
// Prints {"ok", "frames", "error"}; ok = false without a GPU (the adapter's soft failure), exit code 0 either way.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <dgs/odometry_fleet_hip.hpp>

static bool read_all(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const std::string method = argv[1];
  dgs_params prm;
  if (dgs_params_init(&prm, method == "FAST_GICP" ? DGS_METHOD_GICP : method == "GICP_HIP" ? DGS_METHOD_PCL_GICP : method == "NDT_OMP" ? DGS_METHOD_NDT : -1) != DGS_OK) {
    std::printf("{\"error\": \"unknown method\"}\n");
    return 3;
  }
  prm.gicp_max_correspondence_distance = std::atof(argv[5]);
  prm.transformation_epsilon = std::atof(argv[7]);
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  int64_t B = 0, F = 0;
  if (!read_all(f, &B, 8) || B < 1) return 3;
  std::vector<dgs::OdometryStreamParams> sp((size_t)B);
  for (auto& p : sp) {
    double v[6];
    if (!read_all(f, v, sizeof(v))) return 3;
    p.keyframe_delta_trans = v[0]; p.keyframe_delta_angle = v[1]; p.keyframe_delta_time = v[2];
    p.transform_thresholding = v[3] != 0.0; p.max_acceptable_trans = v[4]; p.max_acceptable_angle = v[5];
  }
  if (!read_all(f, &F, 8) || F < 0) return 3;
  dgs::HipOdometryFleet fleet(prm, sp, dgs::HipOdometryFleet::VOXELGRID, (float)std::atof(argv[6]), std::atoi(argv[4]) != 0);
  FILE* o = std::fopen(argv[3], "wb");
  if (!o) return 4;
  bool ok = true;
  int64_t done = 0;
  std::vector<std::vector<float>> pts((size_t)B);
  std::vector<dgs::HipOdometryFleet::Frame> frames((size_t)B);
  std::vector<dgs::HipOdometryFleet::Matrix4> odoms;
  for (int64_t k = 0; k < F && ok; k++) {
    std::vector<int> before((size_t)B);
    for (int64_t i = 0; i < B; i++) {
      int64_t n = 0;
      double stamp = 0.0;
      if (!read_all(f, &n, 8) || !read_all(f, &stamp, 8)) return 3;
      frames[(size_t)i] = dgs::HipOdometryFleet::Frame{};
      if (n >= 0) {
        pts[(size_t)i].resize((size_t)n * 4 + 4);
        if (!read_all(f, pts[(size_t)i].data(), (size_t)n * 16)) return 3;
        frames[(size_t)i].points = pts[(size_t)i].data();
        frames[(size_t)i].n = n;
        frames[(size_t)i].stamp = stamp;
      }
      before[(size_t)i] = fleet.keyframes((size_t)i);
    }
    ok = fleet.step(frames, &odoms, true);
    if (!ok) break;
    for (int64_t i = 0; i < B; i++) {
      const bool registered = frames[(size_t)i].points && before[(size_t)i] > 0;
      dgs::HipOdometryFleet::Status st = registered ? fleet.status((size_t)i) : dgs::HipOdometryFleet::Status{};
      const int32_t flags[2] = {st.has_converged ? 1 : 0, fleet.keyframes((size_t)i)};
      const double figures[2] = {registered ? st.matching_error : 0.0, registered ? st.inlier_fraction : 0.0};
      std::fwrite(odoms[(size_t)i].data(), 4, 16, o);
      std::fwrite(st.relative_pose.data(), 4, 16, o);
      std::fwrite(flags, 4, 2, o);
      std::fwrite(figures, 8, 2, o);
    }
    done++;
  }
  std::fclose(f);
  std::fclose(o);
  std::string err = ok ? "" : fleet.lastError();
  for (char& ch : err)
    if (ch == '"' || ch == '\\' || ch == '\n') ch = ' ';
  std::printf("{\"ok\": %s, \"frames\": %lld, \"error\": \"%s\"}\n", ok ? "true" : "false", (long long)done, err.c_str());
  return 0;
}

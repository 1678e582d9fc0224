// overlap_port.cpp — a stand-alone single-thread C++ port of the mask painting that
// okvisgpu_frame_overlap replaces: ViSlamBackend::overlapFraction (ViSlamBackend.cpp:2903-2989) in the
// loop of mostOverlappedStateId (:2780-2809), both parts of Frontend::doWeNeedANewKeyframe
// (Frontend.cpp:1186-1295) and ViSlamBackend::trackingQuality (ViSlamBackend.cpp:261-300), with byte
// masks, std::set intersections and its own filled-circle rasteriser (the midpoint routine of OpenCV's
// 8-connected Circle(), row by row). It is the CPU figure of scripts/overlap_timing.py: the port on this
// host, not the reference (which needs OpenCV and is not buildable here).
//   g++ -O3 -std=c++17 scripts/overlap_port.cpp -o scripts/overlap_port        (timing)
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 scripts/overlap_port.cpp -o overlap_port_san  (checks)
// Usage: overlap_port FILE FACTOR [REPS]   -> one JSON line
// FILE (written by overlap_timing.py): int32 n_frames, n_images, rows, cols, n_kp, then per image of every
// frame float kp[n_kp][2], uint64 landmark[n_kp], uint8 flag[n_kp]. Frame 0 is the current frame.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <set>
#include <vector>

struct Image {
  int rows, cols;
  std::vector<float> kp;
  std::vector<uint64_t> lm;
  std::vector<uint8_t> flag;
  size_t num() const { return lm.size(); }
};
using Frame = std::vector<Image>;

struct Mat {
  int rows, cols;
  std::vector<uint8_t> d;
  Mat(int r, int c) : rows(r), cols(c), d((size_t)r * (size_t)c, 0) {}
};

static void hline(Mat& m, int y, int x1, int x2) {
  if (y < 0 || y >= m.rows) return;
  x1 = std::max(x1, 0);
  x2 = std::min(x2, m.cols - 1);
  for (int x = x1; x <= x2; ++x) m.d[(size_t)y * m.cols + x] = 255;
}

// cv::circle(img, pt * 0.1, radius, 255, cv::FILLED)
static void circle(Mat& m, const float* pt, int radius) {
  const float fx = (float)((double)pt[0] * 0.1), fy = (float)((double)pt[1] * 0.1);
  if (!(std::fabs(fx) < 1073741824.0f) || !(std::fabs(fy) < 1073741824.0f)) return;
  const int cx = (int)std::nearbyint(fx), cy = (int)std::nearbyint(fy);  // cvRound: ties to even
  int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
  while (dx >= dy) {
    hline(m, cy - dy, cx - dx, cx + dx);
    hline(m, cy + dy, cx - dx, cx + dx);
    hline(m, cy - dx, cx - dy, cx + dy);
    hline(m, cy + dx, cx - dy, cx + dy);
    ++dy;
    err += plus;
    plus += 2;
    if (err > 0) {
      err -= minus;
      --dx;
      minus -= 2;
    }
  }
}

static void iou(const Mat& matches, const Mat& detections, int& inter, int& uni) {
  for (size_t i = 0; i < matches.d.size(); ++i) {
    inter += (matches.d[i] & detections.d[i]) != 0;
    uni += (matches.d[i] | detections.d[i]) != 0;
  }
}

static double overlapFraction(const Frame& A, const Frame& B, double kptradius) {
  const Frame* frames[2] = {&A, &B};
  std::set<uint64_t> landmarks[2];
  std::vector<Mat> det[2], mat[2];
  for (int f = 0; f < 2; ++f)
    for (const Image& im : *frames[f]) {
      const int rows = im.rows / 10, cols = im.cols / 10;
      const double radius = double(std::min(rows, cols)) * kptradius;
      det[f].emplace_back(rows, cols);
      mat[f].emplace_back(rows, cols);
      if (im.rows == 0 || im.cols == 0) continue;
      for (size_t k = 0; k < im.num(); ++k) {
        circle(det[f].back(), &im.kp[2 * k], int(radius));
        if (im.lm[k] != 0) landmarks[f].insert(im.lm[k]);
      }
    }
  std::set<uint64_t> matches;
  std::set_intersection(landmarks[0].begin(), landmarks[0].end(), landmarks[1].begin(), landmarks[1].end(),
                        std::inserter(matches, matches.begin()));
  if (matches.empty()) return 0.0;
  double overlap[2];
  for (int f = 0; f < 2; ++f) {
    int inter = 0, uni = 0;
    for (size_t i = 0; i < frames[f]->size(); ++i) {
      const Image& im = (*frames[f])[i];
      if (im.rows == 0 || im.cols == 0) continue;
      const double radius = double(std::min(im.rows / 10, im.cols / 10)) * kptradius;
      for (size_t k = 0; k < im.num(); ++k)
        if (matches.count(im.lm[k])) circle(mat[f][i], &im.kp[2 * k], int(radius));
      iou(mat[f][i], det[f][i], inter, uni);
    }
    overlap[f] = double(inter) / double(uni);
  }
  return std::min(overlap[0], overlap[1]);
}

// the current-frame part of doWeNeedANewKeyframe; fills lmIds
static double currentOverlap(const Frame& cur, double kptrad, std::set<uint64_t>& lmIds) {
  int inter = 0, uni = 0;
  for (const Image& im : cur) {
    const int rows = im.rows / 10, cols = im.cols / 10;
    Mat matches(rows, cols), detections(rows, cols);
    const double radius = double(std::min(rows, cols)) * kptrad;
    for (size_t k = 0; k < im.num(); ++k) {
      circle(detections, &im.kp[2 * k], int(radius));
      if (im.lm[k] != 0) {
        circle(matches, &im.kp[2 * k], int(radius));
        lmIds.insert(im.lm[k]);
      }
    }
    iou(matches, detections, inter, uni);
  }
  return double(inter) / double(uni);
}

static double otherOverlap(const Frame& other, double kptrad, const std::set<uint64_t>& lmIds) {
  int inter = 0, uni = 0;
  for (const Image& im : other) {
    const int rows = im.rows / 10, cols = im.cols / 10;
    Mat matches(rows, cols), detections(rows, cols);
    const double radius = double(std::min(rows, cols)) * kptrad;
    for (size_t k = 0; k < im.num(); ++k) {
      circle(detections, &im.kp[2 * k], int(radius));
      if (im.lm[k] != 0 && lmIds.count(im.lm[k])) circle(matches, &im.kp[2 * k], int(radius));
    }
    iou(matches, detections, inter, uni);
  }
  return double(inter) / double(uni);
}

static double trackingQuality(const Frame& frame, double kptradius) {
  int inter = 0, uni = 0, matchedPoints = 0;
  for (const Image& im : frame) {
    const int rows = im.rows / 10, cols = im.cols / 10;
    const double radius = double(std::min(rows, cols)) * kptradius;
    Mat matches(rows, cols);
    for (size_t k = 0; k < im.num(); ++k)
      if (im.flag[k]) {
        ++matchedPoints;
        circle(matches, &im.kp[2 * k], int(radius));
      }
    const int pointArea = int(radius * radius * M_PI);
    int painted = 0;
    for (uint8_t v : matches.d) painted += v != 0;
    inter += std::max(0, painted - pointArea);
    uni += rows * cols - pointArea;
  }
  return matchedPoints < 8 ? 0.0 : double(inter) / double(uni);
}

static double medianMs(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: overlap_port FILE FACTOR [REPS]\n");
    return 2;
  }
  const double factor = std::atof(argv[2]);
  const int reps = argc > 3 ? std::atoi(argv[3]) : 5;
  std::FILE* f = std::fopen(argv[1], "rb");
  int32_t head[5];
  if (!f || std::fread(head, 4, 5, f) != 5) return 2;
  const int nf = head[0], ni = head[1], nk = head[4];
  std::vector<Frame> frames((size_t)nf);
  for (Frame& fr : frames)
    for (int i = 0; i < ni; ++i) {
      Image im{head[2], head[3], std::vector<float>(2 * (size_t)nk), std::vector<uint64_t>((size_t)nk),
               std::vector<uint8_t>((size_t)nk)};
      if (std::fread(im.kp.data(), 4, 2 * (size_t)nk, f) != 2 * (size_t)nk || std::fread(im.lm.data(), 8, (size_t)nk, f) != (size_t)nk ||
          std::fread(im.flag.data(), 1, (size_t)nk, f) != (size_t)nk)
        return 2;
      fr.push_back(std::move(im));
    }
  std::fclose(f);
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  std::vector<double> tPairs, tKeyframe, tQuality, pairs((size_t)nf, 0.0), others((size_t)nf, 0.0);
  double current = 0.0, quality = 0.0;
  int best = -1;
  for (int r = 0; r < reps; ++r) {
    auto a = clk::now();
    double overlap = 0.0;  // mostOverlappedStateId(frame 0)
    best = -1;
    for (int k = 1; k < nf; ++k) {
      pairs[(size_t)k] = overlapFraction(frames[(size_t)k], frames[0], factor);
      if (pairs[(size_t)k] >= overlap) {
        best = k;
        overlap = pairs[(size_t)k];
      }
    }
    auto b = clk::now();
    std::set<uint64_t> lmIds;  // doWeNeedANewKeyframe(frame 0)
    current = currentOverlap(frames[0], factor, lmIds);
    for (int k = 1; k < nf; ++k) others[(size_t)k] = otherOverlap(frames[(size_t)k], factor, lmIds);
    auto c = clk::now();
    quality = trackingQuality(frames[0], factor);
    auto d = clk::now();
    tPairs.push_back(ms(a, b));
    tKeyframe.push_back(ms(b, c));
    tQuality.push_back(ms(c, d));
  }
  std::printf("{\"impl\": \"cpp_port_single_thread\", \"frames\": %d, \"images\": %d, \"keypoints\": %d, \"reps\": %d, "
              "\"most_overlapped_ms_median\": %.4f, \"new_keyframe_ms_median\": %.4f, \"tracking_quality_ms_median\": %.4f, "
              "\"best\": %d, \"current\": %.17g, \"quality\": %.17g, \"pairs\": [",
              nf, ni, nk, reps, medianMs(tPairs), medianMs(tKeyframe), medianMs(tQuality), best, current, quality);
  for (int k = 1; k < nf; ++k) std::printf("%s%.17g", k > 1 ? ", " : "", pairs[(size_t)k]);
  std::printf("], \"others\": [");
  for (int k = 1; k < nf; ++k) std::printf("%s%.17g", k > 1 ? ", " : "", others[(size_t)k]);
  std::printf("]}\n");
  return 0;
}

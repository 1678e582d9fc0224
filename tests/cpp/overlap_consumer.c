/* A plain-C consumer of okvisgpu_frame_overlap (C99, -pedantic): fills the batch the way an adapter
 * would (one keyframe against the current frame, two cameras) and calls the entry point.
 * Usage: overlap_consumer       (no GPU: the NULL context is refused)
 *        overlap_consumer gpu   (one kind-0 job and its group on device 0; prints the outputs) */
#include <stdio.h>
#include <string.h>

#include "okvisgpu.h"

int main(int argc, char** argv) {
  const int gpu = argc > 1 && strcmp(argv[1], "gpu") == 0;
  const int32_t image_begin[3] = {0, 2, 4};
  const int32_t rows[4] = {480, 480, 480, 480}, cols[4] = {752, 752, 752, 752};
  const int32_t kp_begin[5] = {0, 2, 3, 5, 6};
  const float keypoint[6][2] = {{100.f, 100.f}, {300.f, 200.f}, {50.f, 60.f}, {110.f, 95.f}, {700.f, 400.f}, {55.f, 66.f}};
  const uint64_t landmark[6] = {7u, 0u, 9u, 7u, 11u, 9u};
  const int32_t job_kind[1] = {0}, job_frame_a[1] = {0}, job_frame_b[1] = {1}, group_begin[2] = {0, 1};
  const double factor[1] = {0.09};
  double overlap[1] = {-1.0}, group_max[1] = {-1.0};
  int32_t count[4] = {-1, -1, -1, -1}, n_matched[2] = {-1, -1}, n_keypoints[1] = {-1}, group_best[1] = {-2};
  okvisgpu_frame_overlap_batch b;
  okvisgpu_frame_overlap_result r;
  okvisgpu_ctx* ctx = NULL;
  int rc;
  memset(&b, 0, sizeof b);
  memset(&r, 0, sizeof r);
  b.n_frames = 2;
  b.image_begin = image_begin;
  b.rows = rows;
  b.cols = cols;
  b.kp_begin = kp_begin;
  b.keypoint = &keypoint[0][0];
  b.landmark = landmark;
  b.n_jobs = 1;
  b.job_kind = job_kind;
  b.job_frame_a = job_frame_a;
  b.job_frame_b = job_frame_b;
  b.job_radius_factor = factor;
  b.n_groups = 1;
  b.group_begin = group_begin;
  r.overlap = overlap;
  r.count = &count[0];
  r.n_matched = &n_matched[0];
  r.n_keypoints = n_keypoints;
  r.group_best = group_best;
  r.group_max = group_max;
  rc = okvisgpu_frame_overlap(NULL, &b, &r);
  if (rc != OKVISGPU_ERR_INVALID_ARGUMENT || overlap[0] != -1.0 || count[0] != -1) {
    fprintf(stderr, "overlap_consumer: the NULL context must be refused and nothing written (%d)\n", rc);
    return 1;
  }
  printf("overlap_consumer: null context refused (masks of %d words, radius up to %d)\n", OKVISGPU_OVERLAP_MASK_WORDS,
         OKVISGPU_OVERLAP_MAX_RADIUS);
  if (!gpu) return 0;
  rc = okvisgpu_ctx_create(0, &ctx);
  if (rc != OKVISGPU_OK) {
    fprintf(stderr, "overlap_consumer: ctx_create failed (%d)\n", rc);
    return 1;
  }
  rc = okvisgpu_frame_overlap(ctx, &b, &r);
  if (rc != OKVISGPU_OK) {
    fprintf(stderr, "overlap_consumer: frame_overlap failed (%d): %s\n", rc, okvisgpu_last_error(ctx));
    okvisgpu_ctx_destroy(ctx);
    return 1;
  }
  printf("{\"overlap\": %.17g, \"count\": [%d, %d, %d, %d], \"n_matched\": [%d, %d], \"n_keypoints\": %d, "
         "\"group_best\": %d, \"group_max\": %.17g}\n",
         overlap[0], count[0], count[1], count[2], count[3], n_matched[0], n_matched[1], n_keypoints[0], group_best[0],
         group_max[0]);
  okvisgpu_ctx_destroy(ctx);
  return 0;
}

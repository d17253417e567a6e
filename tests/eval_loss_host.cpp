// tests/eval_loss_host.cpp -- host build of the test-time criterion's arithmetic (TEST INFRASTRUCTURE).
//
// Compiles the eval_* functions of 3dioumatch_amd/csrc/loss_core.h -- the very functions the gfx950
// kernels eval_decode_kernel / eval_terms_kernel / eval_stats_kernel call -- with the host compiler
// and runs them from plain loops, so that the labels and the 20 statistics of models/loss_helper.py
// get_loss can be compared with a float64 evaluation on a machine without a GPU
// (tests/test_eval_loss.py).  Pointers are HOST pointers here.  Built on demand:
//   g++ -O2 -shared -fPIC -ffp-contract=off -o tests/_eval_loss_host.so tests/eval_loss_host.cpp
// A stand-alone sanitizer run links this file into a program of its own; it is never loaded into
// Python with a sanitizer runtime.
#include <vector>

#include "../3dioumatch_amd/csrc/loss_core.h"

extern "C" int host_eval_loss_scratch_floats(const VnLossArgs *args) {
  return args->B * loss_blocks_per_scene(args->K, args->S) * ACC_COUNT;
}

extern "C" int host_eval_loss_decode(const VnLossArgs *args) {
  const LossArgs &a = *args;
  for (int b = 0; b < a.B; ++b) {
    for (int k = 0; k < a.K; ++k) eval_decode_prediction(a, b, k);
    for (int g = 0; g < a.G; ++g) decode_ground_truth(a, b, g);
  }
  return 0;
}

extern "C" int host_eval_loss(const VnLossArgs *args, float *stats, float *accum) {
  const LossArgs &a = *args;
  float acc[ACC_COUNT] = {};
  std::vector<float> centers((size_t)a.K * 3);
  for (int b = 0; b < a.B; ++b) {
    for (int k = 0; k < a.K; ++k)
      for (int d = 0; d < 3; ++d) centers[k * 3 + d] = lt_at(a.center, b, k, d);
    SceneView sv;
    sv.gt_center = a.center_label + (long long)b * a.G * 3;
    sv.gt_mask = a.box_label_mask + (long long)b * a.G;
    sv.center = centers.data();
    sv.nearest = nullptr;
    for (int k = 0; k < a.K; ++k) eval_proposal(a, sv, b, k, acc);
    for (int g = 0; g < a.G; ++g) eval_ground_truth(a, sv, g, acc);
    for (int s = 0; s < a.S; ++s) {
      float m;
      loss_seed(a, b, s, acc, &m);
    }
  }
  eval_stats(a, acc, stats, accum);
  return 0;
}

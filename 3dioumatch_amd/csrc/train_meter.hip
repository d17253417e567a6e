// 3dioumatch_amd/csrc/train_meter.hip -- the running sums behind the training loop's log lines.
//
// What it replaces: the statistics loop of train_one_epoch (train.py:356-360, pretrain.py:335-339),
// one .item() per logged key and step.  Against a graph-replayed step whose outputs are static
// device scalars the sums are one launch captured behind the Adam call (votenet/train_meter.py).
#include "common.h"

// The training loop's statistics (train.py:356-360) without a host read: accum[i] += *table[i] for
// count device scalars, in double; accum[count] counts the applied steps, accum[count + 1] the
// skipped ones (guard[2] == 1: nothing else is added), accum[count + 2] sums the gradient norm.
namespace {
__global__ void __launch_bounds__(256)
train_meter_add_kernel(int count, const float *const *__restrict__ table,
                       const double *__restrict__ guard, double *__restrict__ accum) {
  if (guard && guard[2] != 0.0) {
    if (threadIdx.x == 0) accum[count + 1] += 1.0;
    return;
  }
  for (int i = threadIdx.x; i < count; i += 256) accum[i] += (double)table[i][0];
  if (threadIdx.x == 0) {
    accum[count] += 1.0;
    if (guard) accum[count + 2] += guard[0];
  }
}
}  // namespace

PN2_API int votenet_train_meter_add(int count, const float *const *table, const double *guard,
                                    double *accum, void *stream_) {
  if (count < 0 || (count > 0 && !table) || !accum) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(train_meter_add_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream_, count, table,
                     guard, accum);
  return pn2_launch_status();
}

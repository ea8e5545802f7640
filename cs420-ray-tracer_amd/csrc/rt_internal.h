// rt_internal.h -- what the translation units of librt_hip.so share beyond the
// C-ABI (include/rt_hip.h).  Not exported: the device group (rt_group.hip)
// reads a member's launches through these without the host waits of
// rt_render_stats / rt_kernel_times and without consuming what they report.
#ifndef RT_INTERNAL_H
#define RT_INTERNAL_H

#include "rt_hip.h"

#define RT_INTERNAL __attribute__((visibility("hidden")))

// u64 slots of an rt_add_counts accumulator: rt_stats' six counters, in its order.
constexpr int kRtCountSlots = 6;

// Enqueues, on the context's stream, acc[q] += counter q of the context's most
// recent launch (summed over its shards), q < kRtCountSlots.  acc is memory of
// the context's device that only this stream writes.  Stream order puts it
// before the next launch, which re-zeroes those counters; the host never waits.
RT_INTERNAL int rt_add_counts(rt_ctx *ctx, unsigned long long *acc_device);

// kernel_ms of launch `index` (0 = the context's first, rt_info.launches - 1 its latest), one of the 256 most
// recent.  Waits for that launch alone, not for the stream, and leaves the
// history of rt_kernel_times as it is.
RT_INTERNAL int rt_launch_ms(rt_ctx *ctx, long long index, double *ms);

// The sample count of the context's light table (rt_set_light_samples); 0 without one.  No HIP call.
RT_INTERNAL int rt_light_samples(const rt_ctx *ctx);
// The same of its gloss table (rt_set_gloss_samples).
RT_INTERNAL int rt_gloss_samples(const rt_ctx *ctx);

#endif  // RT_INTERNAL_H

// ltr_linear.hip -- translation unit of the fused Linear(F,1) scorer + pairwise loss step of libltr_hip.so; compiled next to
// ltr_kernels.hip, ltr_mlp.hip and ltr_linear_bf16.hip (pytorchltr_amd/build.py), so the four build in parallel.  This file is the table of
// contents: the code is in the .inc files below, each of which needs only what stands above it.
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string.h>
#include <thread>

#include "ltr_common.inc"       // the C ABI's codes, the loss kinds' pair passes, the status word, partial_pitch
#include "ltr_sched.h"          // the list-length scheduling of the query workgroups
#include "ltr_linear.inc"       // LinearParams, the general, register-tile and reduction kernels, their shape choosers and launchers
#include "ltr_areas.inc"        // host: the pool of library-owned, zeroed device areas (exchange areas, lazy areas); needs nothing above but the codes
#include "ltr_cluster.inc"      // the cluster kernel (long lists, small batches); needs LinearParams and exchange_area_get
#include "ltr_parts.inc"        // the parts kernel (one query over several workgroups); needs the same, and ltr_cluster.inc's time-out switch
#include "ltr_overlap.inc"      // host: the step's bucket, its collective call and the helper thread that overlaps it; no GPU code
#include "ltr_mailbox.inc"      // the mailbox all-reduce over IPC memory; needs MailboxDev and lazy_area_words (ltr_linear.inc), mailbox_next_tag (ltr_areas.inc)
#include "ltr_linear_step.inc"  // host: the planner, the partials launch, the reduce and step entry points; needs every file above
#include "ltr_linear_lazy.inc"  // host: the lazy SGD step and its flush; needs the step's launch, the mailbox and lazy_area_next

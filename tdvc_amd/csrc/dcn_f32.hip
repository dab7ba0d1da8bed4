// dcn_f32 — tdvc_dcn_fused on fp32 maps: the deformable conv of the whole-model fp32 mode (`enable_amp: False` of the reference,
// VideoCompressor.model_fp32).  It is dcn_fused_kernel<float> (csrc/dcn_common.h, where the fp32 points of the kernel are described),
// instantiated in a file of its own so that it is built without csrc/dcn.hip's -fno-slp-vectorize.
#include "dcn_common.h"

// tdvc_dcn_fused forwards here when d->x.dtype == TDVC_F32 (csrc/dcn.hip), after dcn_validate
int tdvc_dcn_fused_f32(const tdvc_dcn_desc* d, void* stream) { return launch_dcn_fused<float>(d, stream); }

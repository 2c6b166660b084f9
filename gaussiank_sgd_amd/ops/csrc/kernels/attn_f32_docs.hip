// The document-mask (DOC) instantiations of the fp32 fused attention kernels: attn_f32.hip's kernel templates,
// instantiated with DOC alone and launched through attn_f32_doc_launch_fwd / attn_f32_doc_launch_bwd.  A unit
// of its own for the reason attn_docs.hip gives: it is built without the packed fp32 VALU ops.
#define GK_ATTN_DOC_UNIT 1
#include "attn_f32.hip"

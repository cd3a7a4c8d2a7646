// embedding_update_f32.hip -- the fused table update's kernels on fp32 weight rows (emb_reduce.h) and the launcher embedding.hip reaches them through
#include "emb_reduce.h"

namespace ffh_emb {

bool emb_update_launch_f32(const UpdateLaunch& u) { return emb_update_launch<float>(u, std::make_integer_sequence<int, kUpdateEntries>()); }

}  // namespace ffh_emb

// embedding_update_bf16.hip -- the fused table update's kernels on bf16 weight rows (emb_reduce.h) and the launcher embedding.hip reaches them through
#include "emb_reduce.h"

namespace ffh_emb {

bool emb_update_launch_bf16(const UpdateLaunch& u) { return emb_update_launch<uint16_t>(u, std::make_integer_sequence<int, kUpdateEntries>()); }

}  // namespace ffh_emb

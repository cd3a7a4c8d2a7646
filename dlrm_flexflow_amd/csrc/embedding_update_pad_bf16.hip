// embedding_update_pad_bf16.hip -- the pad forms (include/ff_hip_pad.h) of the ragged table update's apply kernels on bf16 weight rows
// (emb_bags_update.h, PAD = true) and the launcher embedding.hip reaches them through
#include "emb_bags_update.h"

namespace ffh_emb {

bool emb_pad_update_launch_bf16(const BagsUpdateLaunch& u) { return emb_bags_update_launch<uint16_t, true>(u, std::make_integer_sequence<int, kUpdateEntries>()); }

}  // namespace ffh_emb

// embedding_update_padmean_bf16.hip -- the mean forms (include/ff_hip_pad_mean.h) of the ragged table update's apply kernels on bf16 weight rows
// (emb_bags_update.h, PAD = MEAN = true) and the launcher embedding.hip reaches them through
#include "emb_bags_update.h"

namespace ffh_emb {

bool emb_padmean_update_launch_bf16(const BagsUpdateLaunch& u) { return emb_bags_update_launch<uint16_t, true, true>(u, std::make_integer_sequence<int, kUpdateEntries>()); }

}  // namespace ffh_emb

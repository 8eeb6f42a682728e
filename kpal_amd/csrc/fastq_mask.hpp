// fastq_mask.hpp -- the quality mask of a FASTQ call, as the host checks it (kpal_text.hip: fq_mask_options), keeps it between
// calls (kpal_ctx) and hands it to the kernels of fastq_kernels.hpp.
#pragma once

namespace kpal {

struct FqMask {
    int min_quality;   // < 0: no mask
    int offset;        // 33 or 64
};

}  // namespace kpal

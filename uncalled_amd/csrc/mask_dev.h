// Repeat masking (include/uncalled_hip.h: unc_mask_*): what k_mask.hip and unc_mask.cpp share.
//
// The text on the device is one byte per base: bits 0..2 the code (0..3 a base, 4 not a base), bit 3 (MASK_CTG_START) set on the
// first base of every contig.  A window [p, p + len) exists iff every byte of it holds a code below 4 and none of the bytes
// behind its first has bit 3 set.  Masking a base writes code 4 and keeps bit 3.  The array is padded with MASK_PAD bytes of code 4
// behind the next multiple of 64, so that a lane reading whole 16-byte quads around its positions stays inside the allocation.
// Occurrence starts / repeat windows are flagged in a bitmap: bit (p & 63) of 64-bit word p >> 6 (little endian: a lane that owns
// the 16 starts of one chunk stores them as one 16-bit word).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unc_dev_types.h"

namespace unc {

constexpr uint8_t MASK_CTG_START = 8;
constexpr uint32_t MASK_RUN = 16;        // window starts per lane of k_kmer_count / k_mask_flag_kmer: one 16-byte quad of the text
constexpr uint32_t MASK_PAD = 64;        // bytes of code 4 behind the text rounded up to a multiple of 64
constexpr uint32_t MASK_MAX_K = 13;
constexpr uint32_t MASK_BLOCK = 256;

// one iteration of internal masking, as the device leaves it
struct MaskIter {
    unsigned long long best;    // count << 32 | (0xFFFFFFFF - k-mer code): the maximum of this word is the largest count, smallest code
    uint32_t occ;               // occurrences flagged
    uint32_t bases;             // bases newly masked
};
// best == 0 until k_kmer_argmax has run; a count below 2 ends the loop: MaskCtl::stop is set and every later kernel returns at once
struct MaskCtl { uint32_t stop, pad; };

void launch_kmer_count(const uint8_t *text, uint64_t n, uint32_t k, uint32_t *counts, const MaskCtl *ctl, uint32_t blocks, hipStream_t st);
void launch_kmer_argmax(const uint32_t *counts, uint64_t n_kmers, MaskIter *it, const MaskCtl *ctl, uint32_t blocks, hipStream_t st);
void launch_mask_flag_kmer(const uint8_t *text, uint64_t n, uint32_t k, MaskIter *it, const MaskCtl *ctl, uint64_t *flags, uint32_t blocks,
                           hipStream_t st);
// it == nullptr: the external mode (no stop flag, newly masked bases added to *bases64)
void launch_mask_cover(uint8_t *text, uint64_t n, uint32_t len, const uint64_t *flags, MaskIter *it, MaskCtl *ctl,
                       unsigned long long *bases64, uint32_t blocks, hipStream_t st);
void launch_fm_window_count(const DevIndex &ix, const uint8_t *text, uint64_t n, uint32_t len, uint64_t min_copy, uint64_t *flags,
                            uint64_t *counts /* null: no tap */, uint32_t blocks, hipStream_t st);

}  // namespace unc

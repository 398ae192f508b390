// What unc_refseq.cpp (host) and k_refseq.hip (kernel) share: the descriptor of one run of reference k-mers and the launch wrapper.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace unc {

// One run of consecutive 5-mers of the packed reference, written to consecutive elements of the output.  Forward: output o is the
// 5-mer that starts at base pac_bit / 2 + o.  Reverse: output o is the reverse complement of the 5-mer that starts at base
// pac_bit / 2 + n - 1 - o.  The host cuts a stretch into runs of about 1024 outputs (unc_refseq.cpp), one wavefront each.
struct RefKmerRun {
    uint64_t pac_bit;             // bit offset of the run's first base in the packed text (two bits a base): 64 bits, GRCh38 has 2^32.5 of them
    uint64_t out_off;             // first output element
    uint32_t n;                   // k-mers
    uint32_t fwd;
};

constexpr uint32_t REF_KMERS_PER_LANE = 16;      // 20 bases = 40 bits, out of three aligned words
constexpr uint32_t REF_PAC_SLACK_WORDS = 2;      // zeroed words behind the last base's word: a lane loads three words from its first base's on

// pac: the packed text as 32-bit words (bytes in file order), REF_PAC_SLACK_WORDS zeroed words behind the last one that holds a base
void launch_ref_kmers(const uint32_t *pac, const RefKmerRun *runs, uint32_t n_runs, uint16_t *out, uint32_t max_blocks, hipStream_t st);
}  // namespace unc

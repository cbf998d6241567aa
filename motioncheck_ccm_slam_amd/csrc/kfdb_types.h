// kfdb_types.h -- argument structures and launchers shared by kfdb_host.cpp and kfdb_kernels.hip (the device KeyFrameDatabase).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "record_types.h"

// Query words the kernel stages in LDS (ids int32 + values double = 12 bytes a word, 24 KiB a workgroup); a longer query is
// searched where it lies in global memory.  ccm_kfdb_query_lds_words() reports it.
#define KFDB_QUERY_LDS_WORDS 2048
#define KFDB_WAVES 4                       // waves (= slots) per workgroup of both kernels

struct KfdbQuery {
    const int32_t* ids;                    // arena
    const double* vals;
    const RecordSlot* slot;                // [n_slots]: offset and length in words
    int32_t n_slots;
    int32_t q_n;                           // the query BowVector, on the device (it may lie inside the arena)
    const int32_t* q_ids;
    const double* q_vals;
    int32_t* words;                        // outputs, [n_slots]
    int32_t* first_word;
    double* score;
};

struct KfdbMove {                          // copies n_jobs entries from one arena into another (growth, compaction)
    const int32_t* src_ids; const double* src_vals;
    int32_t* dst_ids; double* dst_vals;
    const RecordMoveJob* job;
    int32_t n_jobs;
};

void kfdb_launch_query(hipStream_t s, const KfdbQuery& a);
void kfdb_launch_move(hipStream_t s, const KfdbMove& a);

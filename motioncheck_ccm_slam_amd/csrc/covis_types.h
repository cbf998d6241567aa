// covis_types.h -- argument structures and launchers shared by covis_host.cpp and covis_kernels.hip (the device covisibility index).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "record_types.h"

// Features of a query record up to which its hash lives in LDS: cells = the power of two >= 2 * features (load factor <= 0.5), so
// 2048 features take 4096 cells: 16 KiB of keys in k_covis_weights, 32 KiB of keys and counters in k_covis_redundancy.  A longer
// query is hashed in global scratch by k_covis_build.  ccm_covis_lds_features() reports it (CCM_COVIS_LDS_FEATURES lowers it).
#define COVIS_LDS_FEATURES 2048
#define COVIS_WAVES 4                      // waves per workgroup of k_covis_weights, k_covis_build and k_covis_move
#define COVIS_WAVE_RECORDS 4               // stored records a wave of k_covis_weights takes, one after the other
#define COVIS_CHUNK (COVIS_WAVES * COVIS_WAVE_RECORDS)      // stored slots per workgroup of k_covis_weights
#define COVIS_EMPTY (-1)                   // an empty hash cell (a counting slot id is >= 0)
#define COVIS_MAX_TH_OBS (1 << 20)         // th_obs above this is refused: the per-entry counter has 24 bits and stops at th_obs
#define COVIS_MP_LIVE 1                    // CCM_MP_LIVE / CCM_MP_BAD of include/ccm_hot.h (covis_host.cpp asserts the equality)
#define COVIS_MP_BAD 2

struct CovisQ {                            // one query of a launch
    int32_t slot;                          // the stored record that queries
    int32_t cells;                         // hash cells, a power of two >= max(2 * len, 64)
    int64_t hash;                          // >= 0: the hash lies in global scratch at this cell (built by k_covis_build); -1: in LDS
};

struct CovisQuery {
    const int32_t* slots;                  // arena: table slot per feature
    const uint8_t* octave;                 //        octave per feature
    const RecordSlot* slot;                // [n_slots]: offset and length in features
    int32_t n_slots, n_q;
    const CovisQ* q;                       // [n_q]
    const uint8_t* flags;                  // the map-point table's flags column, or nullptr: every entry that holds a point counts
    int32_t flags_capacity;
    int32_t th_obs;
    int32_t* g_key;                        // global hash scratch: keys, and per cell octave << 24 | counter
    int32_t* g_val;
    int32_t* weights;                      // outputs: [n_q][n_slots]
    int32_t* n_mps;                        //          [n_q] each
    int32_t* n_redundant;
    int32_t* skipped;
};

struct CovisMove {                         // copies n_jobs records from one arena into another (growth, compaction)
    const int32_t* src_slots; const uint8_t* src_octave;
    int32_t* dst_slots; uint8_t* dst_octave;
    const RecordMoveJob* job;
    int32_t n_jobs;
};

// lds_cells: the cells of the launch's largest LDS-hashed query (0 when every query is hashed in global scratch)
void covis_launch_build(hipStream_t s, const CovisQuery& a);                     // the global hashes; a no-op for the LDS queries
void covis_launch_weights(hipStream_t s, const CovisQuery& a, int lds_cells);
void covis_launch_redundancy(hipStream_t s, const CovisQuery& a, int lds_cells);
void covis_launch_move(hipStream_t s, const CovisMove& a);

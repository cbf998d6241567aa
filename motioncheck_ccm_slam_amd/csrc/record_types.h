// record_types.h -- the two device-side structures of the keyed record store (record_index.h, record_store.h), shared by the
// kernels of its owners: kfdb_types.h and covis_types.h include it.  Plain C++, nothing from HIP.
#pragma once
#include <cstdint>

struct RecordSlot {                        // one slot of a store as the device sees it
    int64_t off;                           // first element of the record in the arena
    int32_t len;                           // elements of the record; -1 = free slot
    int32_t pad;
};

struct RecordMoveJob { int64_t src, dst; int32_t len, pad; };     // copies one record from one arena into another

static_assert(sizeof(RecordSlot) == 16 && sizeof(RecordMoveJob) == 24, "the kernels index these as 16 and 24 bytes");

// Device-wide scan, sort and select over n items on stream s: the library's one statement of these calls
// (device_primitives.hip). Every function
//   - returns NNRT_OK and launches nothing for n == 0 (a d_count is then not written), and refuses n >= 2^31;
//   - takes its temporary from `scratch`, which only grows: a scratch that holds enough keeps its pointer, one that must
//     grow and holds memory waits for s first (an earlier launch on s may still read it), and nothing else synchronises;
//   - leaves counts on the device (d_count), for the caller to read back with its own error words.
// Sorts and selects are stable. in and out must not overlap.
#pragma once

#include "common.hpp"

namespace nnrt {

using Scratch = DeviceBuffer<uint8_t>;

nnrt_status exclusive_sum(const int* in, int* out, int64_t n, Scratch& scratch, hipStream_t s);
// stream-ordered: allocates the (empty) scratch on s, no synchronisation
nnrt_status exclusive_sum(const int* in, int* out, int64_t n, StreamScratch<uint8_t>& scratch, hipStream_t s);
// the scan, then *total = out[n - 1] + in[n - 1] on the host (0 for n == 0): synchronises s
nnrt_status exclusive_sum_total(const int* in, int* out, int64_t n, Scratch& scratch, hipStream_t s, int64_t* total);

// ascending over key bits [0, end_bit)
nnrt_status sort_keys(const uint64_t* in, uint64_t* out, int64_t n, int end_bit, Scratch& scratch, hipStream_t s);
nnrt_status sort_pairs(const uint64_t* keys_in, uint64_t* keys_out, const int* vals_in, int* vals_out, int64_t n, int end_bit, Scratch& scratch,
                       hipStream_t s);

// out = the in[i] with flags[i] != 0, in order; *d_count = how many
nnrt_status select_flagged(const uint64_t* in, const uint8_t* flags, uint64_t* out, int* d_count, int64_t n, Scratch& scratch, hipStream_t s);
nnrt_status select_flagged(const int64_t* in, const uint8_t* flags, int64_t* out, int64_t* d_count, int64_t n, Scratch& scratch, hipStream_t s);
nnrt_status select_flagged(const int* in, const uint8_t* flags, int* out, int64_t* d_count, int64_t n, Scratch& scratch, hipStream_t s);
// the same over in[i] = i
nnrt_status select_flagged_indices(const uint8_t* flags, int64_t* out, int64_t* d_count, int64_t n, Scratch& scratch, hipStream_t s);

// the first of every run of equal keys
nnrt_status unique_keys(const uint64_t* in, uint64_t* out, int* d_count, int64_t n, Scratch& scratch, hipStream_t s);

} // namespace nnrt

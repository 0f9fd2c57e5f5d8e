// device_primitives.hpp over hipcub: the only file in csrc/ that includes it.
#include <hipcub/hipcub.hpp>

#include "device_primitives.hpp"

namespace nnrt {

namespace {

// The reserve rule. A scratch that holds enough keeps its pointer. One that must grow is released first, and releasing
// memory that an earlier launch on s may still be reading is only safe once s has drained: so wait for s, but only when
// there is something to release.
nnrt_status reserve(Scratch& scratch, size_t bytes, hipStream_t s) {
	if (scratch.ptr && bytes <= scratch.count) return NNRT_OK;
	if (scratch.ptr) NNRT_HIP(hipStreamSynchronize(s));
	return scratch.ensure(bytes);
}
nnrt_status reserve(StreamScratch<uint8_t>& scratch, size_t bytes, hipStream_t s) { return scratch.alloc(bytes, s); }

// query -> reserve -> run: call(temporary, bytes, n) is one hipcub entry point with its arguments bound
template <typename S, typename Call>
nnrt_status run(int64_t n, S& scratch, hipStream_t s, Call call) {
	if (n == 0) return NNRT_OK;
	NNRT_CHECK_ARG(n > 0 && n < (int64_t(1) << 31), "a device scan, sort or select takes fewer than 2^31 items, got " + std::to_string(n));
	size_t bytes = 0;
	NNRT_HIP(call(nullptr, bytes, static_cast<int>(n)));
	const nnrt_status st = reserve(scratch, bytes, s);
	if (st) return st;
	NNRT_HIP(call(scratch.ptr, bytes, static_cast<int>(n)));
	return NNRT_OK;
}

template <typename S>
nnrt_status scan(const int* in, int* out, int64_t n, S& scratch, hipStream_t s) {
	return run(n, scratch, s, [=](void* t, size_t& b, int c) { return hipcub::DeviceScan::ExclusiveSum(t, b, in, out, c, s); });
}

template <typename In, typename T, typename C>
nnrt_status flagged(In in, const uint8_t* flags, T* out, C* d_count, int64_t n, Scratch& scratch, hipStream_t s) {
	return run(n, scratch, s, [=](void* t, size_t& b, int c) { return hipcub::DeviceSelect::Flagged(t, b, in, flags, out, d_count, c, s); });
}

} // namespace

nnrt_status exclusive_sum(const int* in, int* out, int64_t n, Scratch& scratch, hipStream_t s) { return scan(in, out, n, scratch, s); }
nnrt_status exclusive_sum(const int* in, int* out, int64_t n, StreamScratch<uint8_t>& scratch, hipStream_t s) { return scan(in, out, n, scratch, s); }

nnrt_status exclusive_sum_total(const int* in, int* out, int64_t n, Scratch& scratch, hipStream_t s, int64_t* total) {
	*total = 0;
	const nnrt_status st = scan(in, out, n, scratch, s);
	if (st || n == 0) return st;
	int last[2] = {0, 0};
	NNRT_HIP(hipMemcpyAsync(&last[0], out + n - 1, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipMemcpyAsync(&last[1], in + n - 1, sizeof(int), hipMemcpyDeviceToHost, s));
	NNRT_HIP(hipStreamSynchronize(s));
	*total = static_cast<int64_t>(last[0]) + last[1];
	return NNRT_OK;
}

nnrt_status sort_keys(const uint64_t* in, uint64_t* out, int64_t n, int end_bit, Scratch& scratch, hipStream_t s) {
	return run(n, scratch, s, [=](void* t, size_t& b, int c) { return hipcub::DeviceRadixSort::SortKeys(t, b, in, out, c, 0, end_bit, s); });
}
nnrt_status sort_pairs(const uint64_t* keys_in, uint64_t* keys_out, const int* vals_in, int* vals_out, int64_t n, int end_bit, Scratch& scratch,
                       hipStream_t s) {
	return run(n, scratch, s, [=](void* t, size_t& b, int c) {
		return hipcub::DeviceRadixSort::SortPairs(t, b, keys_in, keys_out, vals_in, vals_out, c, 0, end_bit, s);
	});
}

nnrt_status select_flagged(const uint64_t* in, const uint8_t* flags, uint64_t* out, int* d_count, int64_t n, Scratch& scratch, hipStream_t s) {
	return flagged(in, flags, out, d_count, n, scratch, s);
}
nnrt_status select_flagged(const int64_t* in, const uint8_t* flags, int64_t* out, int64_t* d_count, int64_t n, Scratch& scratch, hipStream_t s) {
	return flagged(in, flags, out, d_count, n, scratch, s);
}
nnrt_status select_flagged(const int* in, const uint8_t* flags, int* out, int64_t* d_count, int64_t n, Scratch& scratch, hipStream_t s) {
	return flagged(in, flags, out, d_count, n, scratch, s);
}
nnrt_status select_flagged_indices(const uint8_t* flags, int64_t* out, int64_t* d_count, int64_t n, Scratch& scratch, hipStream_t s) {
	return flagged(hipcub::CountingInputIterator<int64_t>(0), flags, out, d_count, n, scratch, s);
}

nnrt_status unique_keys(const uint64_t* in, uint64_t* out, int* d_count, int64_t n, Scratch& scratch, hipStream_t s) {
	return run(n, scratch, s, [=](void* t, size_t& b, int c) { return hipcub::DeviceSelect::Unique(t, b, in, out, d_count, c, s); });
}

} // namespace nnrt

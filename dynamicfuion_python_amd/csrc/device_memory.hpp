// Device memory ownership for the native library: the only callers of the HIP allocator in csrc/ (included by common.hpp).
//
// DeviceBuffer<T>   a growing buffer from the synchronous allocator; handles and plans hold them as members.
// StreamScratch<T>  one stream-ordered temporary, returned to its stream when the scope ends (early returns included).
// DeviceGuard       selects a device for a scope and restores the caller's.
//
// Both owning types free in their destructors, so neither may have static storage duration: device memory is not to be
// released by static destructors after the HIP runtime has shut down (see arrow_pool() in capi.hip).
#pragma once

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <utility>
#include <vector>

namespace nnrt {

// bytes currently held through DeviceBuffer and StreamScratch, process-wide (nnrt_device_bytes_in_use)
inline std::atomic<int64_t> g_device_bytes_in_use{0};

template <typename T>
struct DeviceBuffer {
	T* ptr = nullptr;
	size_t count = 0;
	DeviceBuffer() = default;
	DeviceBuffer(const DeviceBuffer&) = delete;
	DeviceBuffer& operator=(const DeviceBuffer&) = delete;
	DeviceBuffer(DeviceBuffer&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), count(std::exchange(o.count, 0)) {}
	DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
		if (this != &o) {
			release();
			ptr = std::exchange(o.ptr, nullptr);
			count = std::exchange(o.count, 0);
		}
		return *this;
	}
	~DeviceBuffer() { release(); }
	// room for n elements (at least one). n <= count keeps the allocation, so ptr is stable: captured graphs hold it.
	nnrt_status ensure(size_t n) {
		if (n <= count && ptr) return NNRT_OK;
		release();
		const size_t elems = std::max<size_t>(n, 1);
		const hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), sizeof(T) * elems);
		if (e != hipSuccess) {
			set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e));
			ptr = nullptr;
			return NNRT_ERROR_HIP;
		}
		count = elems;
		g_device_bytes_in_use.fetch_add(static_cast<int64_t>(sizeof(T) * count), std::memory_order_relaxed);
		return NNRT_OK;
	}
	void release() {
		if (ptr) {
			hipFree(ptr);
			g_device_bytes_in_use.fetch_sub(static_cast<int64_t>(sizeof(T) * count), std::memory_order_relaxed);
		}
		ptr = nullptr;
		count = 0;
	}
};

template <typename T>
nnrt_status upload(DeviceBuffer<T>& buf, const std::vector<T>& host) {
	nnrt_status st = buf.ensure(host.size());
	if (st) return st;
	if (!host.empty() && hipMemcpy(buf.ptr, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice) != hipSuccess) {
		set_error("hipMemcpy failed");
		return NNRT_ERROR_HIP;
	}
	return NNRT_OK;
}

// The same two for buffers whose address a captured graph may hold: *moved is set when the pointer changed, a pointer
// lost to a failed allocation included (it is never cleared here, so one flag can watch many buffers).
template <typename T>
nnrt_status ensure(DeviceBuffer<T>& buf, size_t n, bool* moved) {
	const T* old = buf.ptr;
	const nnrt_status st = buf.ensure(n);
	if (buf.ptr != old) *moved = true;
	return st;
}
template <typename T>
nnrt_status upload(DeviceBuffer<T>& buf, const std::vector<T>& host, bool* moved) {
	const T* old = buf.ptr;
	const nnrt_status st = upload(buf, host);
	if (buf.ptr != old) *moved = true;
	return st;
}

template <typename T>
struct StreamScratch {
	T* ptr = nullptr;
	StreamScratch() = default;
	StreamScratch(const StreamScratch&) = delete;
	StreamScratch& operator=(const StreamScratch&) = delete;
	~StreamScratch() {
		if (!ptr) return;
		hipFreeAsync(ptr, stream);
		g_device_bytes_in_use.fetch_sub(static_cast<int64_t>(bytes), std::memory_order_relaxed);
	}
	// n elements (at least one) on stream s; one allocation per object
	nnrt_status alloc(size_t n, hipStream_t s) {
		if (ptr) {
			set_error("StreamScratch allocated twice");
			return NNRT_ERROR_ARGUMENT;
		}
		const size_t want = sizeof(T) * std::max<size_t>(n, 1);
		const hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&ptr), want, s);
		if (e != hipSuccess) {
			set_error(std::string("hipMallocAsync failed: ") + hipGetErrorString(e));
			ptr = nullptr;
			return NNRT_ERROR_HIP;
		}
		stream = s;
		bytes = want;
		g_device_bytes_in_use.fetch_add(static_cast<int64_t>(bytes), std::memory_order_relaxed);
		return NNRT_OK;
	}

private:
	hipStream_t stream = nullptr;
	size_t bytes = 0;
};

struct DeviceGuard {
	int prev = -1;
	explicit DeviceGuard(int device) {
		hipGetDevice(&prev);
		if (device >= 0 && device != prev) hipSetDevice(device);
	}
	DeviceGuard(const DeviceGuard&) = delete;
	DeviceGuard& operator=(const DeviceGuard&) = delete;
	~DeviceGuard() {
		int cur = -1;
		hipGetDevice(&cur);
		if (prev >= 0 && cur != prev) hipSetDevice(prev);
	}
};

} // namespace nnrt

// Host check of csrc/device_memory.hpp (DeviceBuffer, the bytes-in-use counter), with or without a device:
//   - move construction and move assignment leave the source empty and carry pointer and count over;
//   - release() is idempotent;
//   - without a device ensure() returns NNRT_ERROR_HIP, sets the error text and leaves ptr null and count zero;
//   - with a device ensure() succeeds, keeps the pointer while n <= count, allocates at least one element, and the
//     counter follows every allocation and release back to where it started.
// Prints "device_memory_check OK (<mode>)" and returns 0, or the failed expectation and 1.
#include "common.hpp"

#include <cstdio>
#include <string>
#include <type_traits>

namespace nnrt {
static std::string g_error;
void set_error(const std::string& m) { g_error = m; }
const std::string& get_error() { return g_error; }
}   // namespace nnrt

using namespace nnrt;

static int failures = 0;
#define EXPECT(cond)                                                      \
	do {                                                                  \
		if (!(cond)) {                                                    \
			fprintf(stderr, "line %d: expected %s\n", __LINE__, #cond);   \
			failures++;                                                   \
		}                                                                 \
	} while (0)

static_assert(!std::is_copy_constructible_v<DeviceBuffer<float>> && !std::is_copy_assignable_v<DeviceBuffer<float>>, "move-only");
static_assert(std::is_nothrow_move_constructible_v<DeviceBuffer<float>> && std::is_nothrow_move_assignable_v<DeviceBuffer<float>>, "movable");
static_assert(!std::is_copy_constructible_v<StreamScratch<int>> && !std::is_move_constructible_v<StreamScratch<int>>, "scope-bound");

static int64_t in_use() { return g_device_bytes_in_use.load(); }

int main() {
	int devices = 0;
	const bool have_device = hipGetDeviceCount(&devices) == hipSuccess && devices > 0;
	const int64_t base = in_use();
	{
		DeviceBuffer<float> a;
		EXPECT(a.ptr == nullptr && a.count == 0);
		a.release();   // empty: nothing to do
		a.release();
		EXPECT(a.ptr == nullptr && a.count == 0 && in_use() == base);
		g_error.clear();
		const nnrt_status st = a.ensure(100);
		if (!have_device) {
			EXPECT(st == NNRT_ERROR_HIP);
			EXPECT(!g_error.empty());
			EXPECT(a.ptr == nullptr && a.count == 0);
			EXPECT(in_use() == base);
			// moves of empty buffers stay empty
			DeviceBuffer<float> b(std::move(a));
			EXPECT(b.ptr == nullptr && b.count == 0 && a.ptr == nullptr && a.count == 0);
			a = std::move(b);
			EXPECT(a.ptr == nullptr && a.count == 0 && b.ptr == nullptr && b.count == 0);
		} else {
			EXPECT(st == NNRT_OK);
			EXPECT(a.ptr != nullptr && a.count == 100);
			EXPECT(in_use() == base + 400);
			float* const p = a.ptr;
			EXPECT(a.ensure(40) == NNRT_OK && a.ptr == p && a.count == 100);    // n <= count: the allocation stays
			EXPECT(a.ensure(100) == NNRT_OK && a.ptr == p && a.count == 100);
			EXPECT(in_use() == base + 400);
			DeviceBuffer<float> b(std::move(a));   // move construction
			EXPECT(a.ptr == nullptr && a.count == 0 && b.ptr == p && b.count == 100);
			EXPECT(in_use() == base + 400);
			DeviceBuffer<float> c;
			EXPECT(c.ensure(0) == NNRT_OK && c.ptr != nullptr && c.count == 1);   // at least one element
			EXPECT(in_use() == base + 404);
			c = std::move(b);   // move assignment: c's own element goes, b's allocation arrives
			EXPECT(b.ptr == nullptr && b.count == 0 && c.ptr == p && c.count == 100);
			EXPECT(in_use() == base + 400);
			EXPECT(c.ensure(101) == NNRT_OK && c.count == 101);   // growth reallocates
			EXPECT(in_use() == base + 404);
			c.release();
			c.release();   // idempotent
			EXPECT(c.ptr == nullptr && c.count == 0 && in_use() == base);
			{
				DeviceBuffer<double> d;
				EXPECT(d.ensure(8) == NNRT_OK && in_use() == base + 64);
			}   // the destructor releases
			EXPECT(in_use() == base);
			{
				StreamScratch<int> s;
				EXPECT(s.alloc(3, nullptr) == NNRT_OK && s.ptr != nullptr && in_use() == base + 12);
				EXPECT(s.alloc(3, nullptr) == NNRT_ERROR_ARGUMENT);   // one allocation per object
			}
			EXPECT(hipStreamSynchronize(nullptr) == hipSuccess);
			EXPECT(in_use() == base);
		}
	}
	EXPECT(in_use() == base);
	if (failures) return 1;
	printf("device_memory_check OK (%s)\n", have_device ? "device" : "no device");
	return 0;
}

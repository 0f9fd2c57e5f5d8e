// Check of csrc/device_primitives.hpp, linked with csrc/device_primitives.hip directly.
//   device_primitives_check host     needs no device:
//     - n == 0 returns NNRT_OK, sets no error and leaves an empty scratch empty;
//     - n == 2^31 (and n < 0) is refused with NNRT_ERROR_ARGUMENT and an error text, the scratch still empty.
//   device_primitives_check device   every function against the host's std::exclusive_scan, std::stable_sort,
//     std::copy_if and std::unique at n = 1, 63, 64, 65, 1023, 1024, 1025, 100003 (one element, each side of a wave, each
//     side of a workgroup, several tiles): sort keys drawn below 2^end_bit for end_bit = 64 and 63; flags all-zero,
//     all-one and mixed; a unique input with a run across index 1024; and the reserve rule: one scratch used large ->
//     small -> larger keeps its pointer on the second call, and the bytes-in-use counter returns to its start.
// Prints "device_primitives_check OK (<mode>)" and returns 0, or the failed expectations and 1.
#include "device_primitives.hpp"

#include <algorithm>
#include <cstdio>
#include <iterator>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

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
#define EXPECT_N(cond, n)                                                                           \
	do {                                                                                            \
		if (!(cond)) {                                                                              \
			fprintf(stderr, "line %d (n = %lld): expected %s\n", __LINE__, (long long)(n), #cond);   \
			failures++;                                                                             \
		}                                                                                           \
	} while (0)

static int64_t in_use() { return g_device_bytes_in_use.load(); }

// ------------------------------------------------------------------ host ----
// every function at item count n with null data: none may touch a pointer, the scratch or the device
template <typename Check>
static void each_function(int64_t n, Check check) {
	DeviceBuffer<uint8_t> scratch;
	StreamScratch<uint8_t> stream_scratch;
	int64_t total = -1;
	check(exclusive_sum(nullptr, nullptr, n, scratch, nullptr));
	check(exclusive_sum(nullptr, nullptr, n, stream_scratch, nullptr));
	check(exclusive_sum_total(nullptr, nullptr, n, scratch, nullptr, &total));
	EXPECT(total == 0);
	check(sort_keys(nullptr, nullptr, n, 64, scratch, nullptr));
	check(sort_pairs(nullptr, nullptr, nullptr, nullptr, n, 63, scratch, nullptr));
	check(select_flagged(static_cast<const uint64_t*>(nullptr), nullptr, static_cast<uint64_t*>(nullptr), static_cast<int*>(nullptr), n, scratch, nullptr));
	check(select_flagged(static_cast<const int64_t*>(nullptr), nullptr, static_cast<int64_t*>(nullptr), static_cast<int64_t*>(nullptr), n, scratch, nullptr));
	check(select_flagged(static_cast<const int*>(nullptr), nullptr, static_cast<int*>(nullptr), static_cast<int64_t*>(nullptr), n, scratch, nullptr));
	check(select_flagged_indices(nullptr, nullptr, nullptr, n, scratch, nullptr));
	check(unique_keys(nullptr, nullptr, nullptr, n, scratch, nullptr));
	EXPECT(scratch.ptr == nullptr && scratch.count == 0 && stream_scratch.ptr == nullptr);
}

static void check_host() {
	const int64_t base = in_use();
	g_error.clear();
	each_function(0, [](nnrt_status st) { EXPECT(st == NNRT_OK && g_error.empty()); });
	for (const int64_t n : {int64_t(1) << 31, (int64_t(1) << 31) + 5, int64_t(-1)}) {
		each_function(n, [](nnrt_status st) {
			EXPECT(st == NNRT_ERROR_ARGUMENT && !g_error.empty());
			g_error.clear();
		});
	}
	EXPECT(in_use() == base);
}

// ---------------------------------------------------------------- device ----
#define HIP_OK(expr) EXPECT((expr) == hipSuccess)

template <typename T>
struct Dev {
	DeviceBuffer<T> buf;
	explicit Dev(size_t n) { EXPECT(buf.ensure(n) == NNRT_OK); }
	explicit Dev(const std::vector<T>& h) {
		EXPECT(buf.ensure(h.size()) == NNRT_OK);
		HIP_OK(hipMemcpy(buf.ptr, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
	}
	std::vector<T> host(size_t n) const {
		std::vector<T> h(n);
		if (n) HIP_OK(hipMemcpy(h.data(), buf.ptr, sizeof(T) * n, hipMemcpyDeviceToHost));
		return h;
	}
	T* ptr() const { return buf.ptr; }
};

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // xorshift64*
	g_rng ^= g_rng >> 12;
	g_rng ^= g_rng << 25;
	g_rng ^= g_rng >> 27;
	return g_rng * 0x2545f4914f6cdd1dull;
}

static void check_scan(int64_t n, hipStream_t s) {
	std::vector<int> in(n), want(n);
	for (auto& v : in) v = static_cast<int>(rnd() % 7);
	std::exclusive_scan(in.begin(), in.end(), want.begin(), 0);
	const int64_t want_total = std::accumulate(in.begin(), in.end(), int64_t(0));
	Dev<int> d_in(in), d_out(n);
	{
		DeviceBuffer<uint8_t> scratch;
		EXPECT_N(exclusive_sum(d_in.ptr(), d_out.ptr(), n, scratch, s) == NNRT_OK, n);
		HIP_OK(hipStreamSynchronize(s));
		EXPECT_N(d_out.host(n) == want, n);
		HIP_OK(hipMemset(d_out.ptr(), 0xff, sizeof(int) * n));
		int64_t total = -1;
		EXPECT_N(exclusive_sum_total(d_in.ptr(), d_out.ptr(), n, scratch, s, &total) == NNRT_OK, n);
		EXPECT_N(total == want_total && d_out.host(n) == want, n);
	}
	{
		HIP_OK(hipMemset(d_out.ptr(), 0xff, sizeof(int) * n));
		StreamScratch<uint8_t> scratch;
		EXPECT_N(exclusive_sum(d_in.ptr(), d_out.ptr(), n, scratch, s) == NNRT_OK && scratch.ptr != nullptr, n);
		HIP_OK(hipStreamSynchronize(s));
		EXPECT_N(d_out.host(n) == want, n);
	}
}

static void check_sort(int64_t n, int end_bit, hipStream_t s) {
	// every other key from few distinct ones (many ties: stability shows in the values), the rest from all of
	// [0, 2^end_bit); the top bit below end_bit is set in some of either kind
	const uint64_t mask = end_bit == 64 ? ~0ull : (1ull << end_bit) - 1;
	std::vector<uint64_t> keys(n);
	for (int64_t i = 0; i < n; i++) keys[i] = (i % 2 ? rnd() : (rnd() % 5) << (end_bit - 3) | rnd() % 3) & mask;
	std::vector<int> vals(n);
	std::iota(vals.begin(), vals.end(), 0);
	std::vector<uint64_t> want_keys = keys;
	std::stable_sort(want_keys.begin(), want_keys.end());
	std::vector<int> want_vals = vals;
	std::stable_sort(want_vals.begin(), want_vals.end(), [&](int a, int b) { return keys[a] < keys[b]; });
	Dev<uint64_t> d_keys(keys), d_keys_out(n);
	Dev<int> d_vals(vals), d_vals_out(n);
	DeviceBuffer<uint8_t> scratch;
	EXPECT_N(sort_keys(d_keys.ptr(), d_keys_out.ptr(), n, end_bit, scratch, s) == NNRT_OK, n);
	HIP_OK(hipStreamSynchronize(s));
	EXPECT_N(d_keys_out.host(n) == want_keys, n);
	HIP_OK(hipMemset(d_keys_out.ptr(), 0xff, sizeof(uint64_t) * n));
	EXPECT_N(sort_pairs(d_keys.ptr(), d_keys_out.ptr(), d_vals.ptr(), d_vals_out.ptr(), n, end_bit, scratch, s) == NNRT_OK, n);
	HIP_OK(hipStreamSynchronize(s));
	EXPECT_N(d_keys_out.host(n) == want_keys && d_vals_out.host(n) == want_vals, n);
}

// flag_mode 0: all zero, 1: all one, 2: mixed
static void check_select(int64_t n, int flag_mode, hipStream_t s) {
	std::vector<uint8_t> flags(n);
	for (auto& f : flags) f = flag_mode == 2 ? static_cast<uint8_t>(rnd() % 3 == 0) : static_cast<uint8_t>(flag_mode);
	std::vector<uint64_t> in_u(n);
	std::vector<int64_t> in_l(n), index(n);
	std::vector<int> in_i(n);
	for (int64_t i = 0; i < n; i++) {
		in_u[i] = rnd();
		in_l[i] = static_cast<int64_t>(rnd());
		in_i[i] = static_cast<int>(rnd());
		index[i] = i;
	}
	auto kept = [&](const auto& in) {
		std::decay_t<decltype(in)> out;
		int64_t i = 0;
		std::copy_if(in.begin(), in.end(), std::back_inserter(out), [&](const auto&) { return flags[i++] != 0; });
		return out;
	};
	const auto want_u = kept(in_u);
	const auto want_l = kept(in_l);
	const auto want_i = kept(in_i);
	const auto want_index = kept(index);
	const size_t m = want_u.size();
	Dev<uint8_t> d_flags(flags);
	Dev<uint64_t> d_in_u(in_u), d_out_u(n);
	Dev<int64_t> d_in_l(in_l), d_out_l(n), d_count_l(std::vector<int64_t>{-1});
	Dev<int> d_in_i(in_i), d_out_i(n), d_count_i(std::vector<int>{-1});
	DeviceBuffer<uint8_t> scratch;
	EXPECT_N(select_flagged(d_in_u.ptr(), d_flags.ptr(), d_out_u.ptr(), d_count_i.ptr(), n, scratch, s) == NNRT_OK, n);
	HIP_OK(hipStreamSynchronize(s));
	EXPECT_N(d_count_i.host(1)[0] == static_cast<int>(m) && d_out_u.host(m) == want_u, n);
	EXPECT_N(select_flagged(d_in_l.ptr(), d_flags.ptr(), d_out_l.ptr(), d_count_l.ptr(), n, scratch, s) == NNRT_OK, n);
	HIP_OK(hipStreamSynchronize(s));
	EXPECT_N(d_count_l.host(1)[0] == static_cast<int64_t>(m) && d_out_l.host(m) == want_l, n);
	HIP_OK(hipMemset(d_count_l.ptr(), 0xff, sizeof(int64_t)));
	EXPECT_N(select_flagged(d_in_i.ptr(), d_flags.ptr(), d_out_i.ptr(), d_count_l.ptr(), n, scratch, s) == NNRT_OK, n);
	HIP_OK(hipStreamSynchronize(s));
	EXPECT_N(d_count_l.host(1)[0] == static_cast<int64_t>(m) && d_out_i.host(m) == want_i, n);
	HIP_OK(hipMemset(d_count_l.ptr(), 0xff, sizeof(int64_t)));
	EXPECT_N(select_flagged_indices(d_flags.ptr(), d_out_l.ptr(), d_count_l.ptr(), n, scratch, s) == NNRT_OK, n);
	HIP_OK(hipStreamSynchronize(s));
	EXPECT_N(d_count_l.host(1)[0] == static_cast<int64_t>(m) && d_out_l.host(m) == want_index, n);
}

static void check_unique(int64_t n, hipStream_t s) {
	// ascending runs of 1..4 equal keys, and one run over [1000, 1050) where n reaches it: it crosses index 1024
	std::vector<uint64_t> in(n);
	uint64_t key = 0;
	for (int64_t i = 0; i < n;) {
		key += 1 + rnd() % 1000;
		int64_t run = 1 + static_cast<int64_t>(rnd() % 4);
		if (i <= 1000 && i + run > 1000) run = 1050 - i;
		for (int64_t j = 0; j < run && i < n; j++) in[i++] = key;
	}
	if (n > 1025) EXPECT(in[1000] == in[1049] && in[1023] == in[1024]);
	std::vector<uint64_t> want = in;
	want.erase(std::unique(want.begin(), want.end()), want.end());
	Dev<uint64_t> d_in(in), d_out(n);
	Dev<int> d_count(std::vector<int>{-1});
	DeviceBuffer<uint8_t> scratch;
	EXPECT_N(unique_keys(d_in.ptr(), d_out.ptr(), d_count.ptr(), n, scratch, s) == NNRT_OK, n);
	HIP_OK(hipStreamSynchronize(s));
	EXPECT_N(d_count.host(1)[0] == static_cast<int>(want.size()) && d_out.host(want.size()) == want, n);
}

// one scratch, large -> small -> larger: the pointer stays on the second call and may change only on the third
static void check_reserve(hipStream_t s) {
	const int64_t base = in_use();
	const int64_t large = 100003, small = 65, larger = 1000003;
	std::vector<uint64_t> keys(larger);
	for (auto& k : keys) k = rnd();
	{
		Dev<uint64_t> d_in(keys), d_out(larger);
		const int64_t held = in_use();
		DeviceBuffer<uint8_t> scratch;
		EXPECT(sort_keys(d_in.ptr(), d_out.ptr(), large, 64, scratch, s) == NNRT_OK);
		const uint8_t* const first = scratch.ptr;
		const size_t first_bytes = scratch.count;
		EXPECT(first != nullptr && in_use() == held + static_cast<int64_t>(first_bytes));
		EXPECT(sort_keys(d_in.ptr(), d_out.ptr(), small, 64, scratch, s) == NNRT_OK);
		EXPECT(scratch.ptr == first && scratch.count == first_bytes);
		EXPECT(sort_keys(d_in.ptr(), d_out.ptr(), larger, 64, scratch, s) == NNRT_OK);
		EXPECT(scratch.count > first_bytes && in_use() == held + static_cast<int64_t>(scratch.count));
		HIP_OK(hipStreamSynchronize(s));
		std::vector<uint64_t> want = keys;
		std::stable_sort(want.begin(), want.end());
		EXPECT(d_out.host(larger) == want);   // the sort that ran in the regrown scratch
		scratch.release();
		EXPECT(in_use() == held);
	}
	EXPECT(in_use() == base);
}

static void check_device() {
	const int64_t base = in_use();
	hipStream_t s = nullptr;
	HIP_OK(hipStreamCreate(&s));
	for (const int64_t n : {int64_t(1), int64_t(63), int64_t(64), int64_t(65), int64_t(1023), int64_t(1024), int64_t(1025), int64_t(100003)}) {
		check_scan(n, s);
		check_sort(n, 64, s);
		check_sort(n, 63, s);
		for (int mode = 0; mode < 3; mode++) check_select(n, mode, s);
		check_unique(n, s);
	}
	check_reserve(s);
	HIP_OK(hipStreamSynchronize(s));
	HIP_OK(hipStreamDestroy(s));
	EXPECT(in_use() == base);
}

int main(int argc, char** argv) {
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "host") check_host();
	else if (mode == "device") check_device();
	else {
		fprintf(stderr, "usage: device_primitives_check host|device\n");
		return 2;
	}
	if (failures) return 1;
	printf("device_primitives_check OK (%s)\n", mode.c_str());
	return 0;
}

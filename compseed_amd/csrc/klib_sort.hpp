// klib_sort.hpp -- klib's introsort (cstl/ksort.h:146-226, ks_introsort) restated as a template.  The reference sorts chains by weight and
// alignment regions by end position / score with it; the sort is not stable, the keys tie often, and what happens next depends on the
// order among equal keys -- so the same steps are taken here: median of first / middle+1 / last as pivot, parked at the end; partitions of
// 16 or fewer elements left alone and finished by ONE insertion sort over the whole array; comb sort (shrink factor 1.2473..., gaps 9
// and 10 replaced by 11) for a partition reached after 2 log2(n) levels.  `lt(a, b)`: a sorts before b.
// The header is also compiled for the device (chain_filter_gpu.hip sorts a read's chains in a kernel, one lane per read): no allocation and
// no std:: call.  The stack of pending partitions is a fixed array: the larger part is the one pushed and the smaller one is continued
// with, so every push at least halves what is left and 64 frames (plus klib's two) hold for any n a size_t can count.
#pragma once
#include <cstddef>

#ifdef __HIP__
#define CS_KLIB_HD __host__ __device__
#else
#define CS_KLIB_HD
#endif

template <class T> CS_KLIB_HD inline void cs_klib_swap_(T &a, T &b) { const T tmp = a; a = b; b = tmp; }
template <class T, class Lt> CS_KLIB_HD void cs_klib_insertion_(T *s, T *t, Lt lt)
{
	for (T *i = s + 1; i < t; ++i)
		for (T *j = i; j > s && lt(*j, *(j - 1)); --j) cs_klib_swap_(*j, *(j - 1));
}
template <class T, class Lt> CS_KLIB_HD void cs_klib_combsort_(size_t n, T *a, Lt lt)
{
	const double shrink = 1.2473309501039786540366528676643;
	size_t gap = n; bool swapped;
	do {
		if (gap > 2) { gap = (size_t)((double)gap / shrink); if (gap == 9 || gap == 10) gap = 11; }
		swapped = false;
		for (T *i = a; i < a + n - gap; ++i) if (lt(i[gap], *i)) { cs_klib_swap_(*i, i[gap]); swapped = true; }
	} while (swapped || gap > 2);
	if (gap != 1) cs_klib_insertion_(a, a + n, lt);
}
template <class T, class Lt> CS_KLIB_HD void cs_klib_introsort(size_t n, T *a, Lt lt)
{
	if (n < 1) return;
	if (n == 2) { if (lt(a[1], a[0])) cs_klib_swap_(a[0], a[1]); return; }
	int d = 2;
	while ((1ul << d) < n) ++d;
	struct Frame { T *lo, *hi; int depth; };
	Frame stack[sizeof(size_t) * 8 + 2]; int top = 0;
	T *s = a, *t = a + (n - 1);
	d <<= 1;
	for (;;) {
		if (s < t) {
			if (--d == 0) { cs_klib_combsort_((size_t)(t - s) + 1, s, lt); t = s; continue; }
			T *i = s, *j = t, *k = i + ((j - i) >> 1) + 1;
			if (lt(*k, *i)) { if (lt(*k, *j)) k = j; }
			else k = lt(*j, *i) ? i : j;
			const T pivot = *k;
			if (k != t) cs_klib_swap_(*k, *t);
			for (;;) {
				do ++i; while (lt(*i, pivot));
				do --j; while (i <= j && lt(pivot, *j));
				if (j <= i) break;
				cs_klib_swap_(*i, *j);
			}
			cs_klib_swap_(*i, *t);
			if (i - s > t - i) {
				if (i - s > 16) stack[top++] = {s, i - 1, d};
				s = t - i > 16 ? i + 1 : t;
			} else {
				if (t - i > 16) stack[top++] = {i + 1, t, d};
				t = i - s > 16 ? i - 1 : s;
			}
		} else {
			if (top == 0) { cs_klib_insertion_(a, a + n, lt); return; }
			--top; s = stack[top].lo; t = stack[top].hi; d = stack[top].depth;
		}
	}
}

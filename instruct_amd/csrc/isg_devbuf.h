/*
 * isg_devbuf.h -- the owners of device and pinned host memory: the only place that allocates and frees either.
 *
 * Contexts hold DevBuf / PinnedBuf members; the kernel-argument structs (DevView, PolyDev, WkWalkArgs, ...) stay plain structs of raw
 * pointers, filled from the owners.  Members return hipError_t and are used inside HIPCHK; a failed call leaves the buffer empty.
 */
#ifndef ISG_DEVBUF_H
#define ISG_DEVBUF_H
#include <hip/hip_runtime.h>
#include <atomic>
#include <vector>

/* allocations alive in this process (isg_diag_live_buffers): +1 per successful allocation, -1 per free */
inline std::atomic<long> g_live_buffers{0};

template <class T, bool PINNED>
struct OwnedBuf {
	OwnedBuf() = default;
	OwnedBuf(const OwnedBuf &) = delete;
	OwnedBuf &operator=(const OwnedBuf &) = delete;
	OwnedBuf(OwnedBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	OwnedBuf &operator=(OwnedBuf &&o) noexcept
	{
		if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
		return *this;
	}
	~OwnedBuf() { reset(); }

	T *get() const { return p_; }
	operator T *() const { return p_; }
	size_t cap() const { return cap_; } /* elements */
	void reset()
	{
		if (p_) {
			(void)(PINNED ? hipHostFree(p_) : hipFree(p_));
			g_live_buffers.fetch_sub(1);
		}
		p_ = nullptr;
		cap_ = 0;
	}
	hipError_t alloc(size_t n)
	{
		reset();
		void *v = nullptr;
		const hipError_t e = PINNED ? hipHostMalloc(&v, sizeof(T) * n, hipHostMallocDefault) : hipMalloc(&v, sizeof(T) * n);
		if (e != hipSuccess) return e;
		p_ = (T *)v;
		cap_ = n;
		if (p_) g_live_buffers.fetch_add(1);
		return hipSuccess;
	}
	hipError_t alloc_zero(size_t n)
	{
		const hipError_t e = alloc(n);
		return e != hipSuccess ? e : hipMemset(p_, 0, sizeof(T) * n);
	}
	/* a zeroed allocation, then a synchronous copy of n elements from the host */
	hipError_t upload(const T *src, size_t n)
	{
		const hipError_t e = alloc_zero(n);
		return e != hipSuccess ? e : hipMemcpy(p_, src, sizeof(T) * n, hipMemcpyHostToDevice);
	}
	template <class A> hipError_t upload(const std::vector<T, A> &v) { return upload(v.data(), v.size()); }
	/* room for at least n elements; what a smaller buffer held is not kept */
	hipError_t grow(size_t n) { return n > cap_ ? alloc(n) : hipSuccess; }

private:
	T *p_ = nullptr;
	size_t cap_ = 0;
};
template <class T> using DevBuf = OwnedBuf<T, false>;
template <class T> using PinnedBuf = OwnedBuf<T, true>;

/* an event created on first use */
struct DevEvent {
	hipEvent_t e = nullptr;
	DevEvent() = default;
	DevEvent(const DevEvent &) = delete;
	DevEvent &operator=(DevEvent &&o) noexcept { reset(); e = o.e; o.e = nullptr; return *this; }
	~DevEvent() { reset(); }
	void reset() { if (e) (void)hipEventDestroy(e); e = nullptr; }
	operator hipEvent_t() const { return e; }
};
#endif

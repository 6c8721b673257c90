// r8b_devblock.h -- a block of device memory with one owner (host only: the engine's stages, r8b_engine.h, and the meters
// of the C ABI layer, r8b_meters.h).  Null until first allocated; freed by its destructor, on whatever device is current
// then -- the engine sees to it that this is the object's own (Engine::StageDevs).
#ifndef R8B_DEVBLOCK_H
#define R8B_DEVBLOCK_H

#include <cstddef>
#include <utility>
#include <vector>

#include "r8b_launch.h"

namespace r8bhip {

template<class T>
struct DevBlock
{
	T* p = nullptr;
	DevBlock() = default;
	DevBlock(const DevBlock&) = delete;
	DevBlock& operator=(const DevBlock&) = delete;
	// (moved from: null.  Assignment exchanges, and what this block held goes with `o`)
	DevBlock(DevBlock&& o) noexcept : p(o.p) { o.p = nullptr; }
	DevBlock& operator=(DevBlock&& o) noexcept { std::swap(p, o.p); return *this; }
	~DevBlock() { dev_free(p); }
	operator T*() const { return p; }
	void reset()
	{
		dev_free(p);
		p = nullptr;
	}
	// (zeroed; whatever it held is freed first)
	void alloc(size_t bytes)
	{
		reset();
		p = (T*) dev_alloc(bytes);
	}
	// a host table as it stands (synchronous); an empty one leaves no block
	template<class U>
	void upload(const std::vector<U>& v)
	{
		if (v.empty()) return reset();
		alloc(v.size() * sizeof(U));
		dev_upload(p, v.data(), v.size() * sizeof(U));
	}
};

} // namespace r8bhip

#endif

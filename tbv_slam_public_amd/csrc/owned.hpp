// owned.hpp -- the one shape every long-lived resource of the library is owned through: a std::unique_ptr whose stateless
// deleter calls a free function and ignores what it returns.  Nothing here names the HIP runtime (common.hpp binds the
// shape to hipFree, hipHostFree, hipEventDestroy, ...), so a host-only program can bind it to a stand-in.
#pragma once
#include <memory>

template <auto Free>
struct FreeWith {
  template <class T> void operator()(T* p) const { (void)Free(p); }
};
// T[] owns an array and indexes it on the host (pinned memory); a plain T is only ever handed on through get()
template <class T, auto Free>
using Owned = std::unique_ptr<T, FreeWith<Free>>;

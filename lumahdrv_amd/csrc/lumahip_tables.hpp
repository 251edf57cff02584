// lumahip_tables.hpp -- what every per-stream table of a context is made of: an owning device buffer, a process-wide cache of
// the host-side build, a per-context LRU of device copies.  A new table is a key, a builder and a size (lumahip_core.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

namespace lhost {

// Keys compare by their bits: -0.0f and 0.0f, or two NaNs of different payload, are different tables
template <typename K>
inline bool same_bits(const K &a, const K &b)
{
    static_assert(std::is_trivially_copyable_v<K>, "a key of plain floats, without padding");
    return memcmp(&a, &b, sizeof(K)) == 0;
}
inline bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

// A table in device memory and its owner: move-only, freed with its owner.  hipFree waits for the device, so whatever still
// reads the table has finished when the memory goes.
template <typename T>
class DevTable {
public:
    T *get() const { return p_.get(); }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() { p_.reset(); }
    // `count` uninitialised elements in a NEW buffer, which replaces the old one only on success
    hipError_t alloc(size_t count)
    {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e == hipSuccess)
            p_.reset(static_cast<T *>(p));
        return e;
    }
    // host[0, count) followed by `fill` up to `padded` elements (the kernels stage tables in 16-byte pieces), with a blocking
    // copy into a NEW buffer, which replaces the old one only on success: a failed upload leaves the table as it was
    hipError_t upload(const T *host, size_t count, size_t padded, T fill)
    {
        std::vector<T> h(padded, fill);
        memcpy(h.data(), host, count * sizeof(T));
        DevTable fresh;
        hipError_t e = fresh.alloc(padded);
        if (e == hipSuccess)
            e = hipMemcpy(fresh.get(), h.data(), padded * sizeof(T), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            *this = std::move(fresh);
        return e;
    }

private:
    struct Free {
        void operator()(T *p) const { (void)hipFree(p); }
    };
    std::unique_ptr<T, Free> p_;
};

// Process-wide cache of host-side tables that are pure functions of their key: several contexts of one process usually hold the
// same table (one per GPU in the multi-device layer, encoder + decoder of a transcoder): built once, shared.  Eight entries,
// the oldest goes first.  The mutex is held across the build, so that contexts that ask at the same time build once; a builder
// must not ask another cache.
template <typename Key, typename Value>
class KeyedCache {
public:
    template <typename Build>
    Value get(const Key &key, Build build)
    {
        std::lock_guard<std::mutex> lk(m_);
        for (const auto &e : e_)
            if (same_bits(e.first, key))
                return e.second;
        Value v = build();
        if (e_.size() >= CAPACITY)
            e_.erase(e_.begin());
        e_.emplace_back(key, v);
        return v;
    }

private:
    static constexpr size_t CAPACITY = 8;
    std::mutex m_;
    std::vector<std::pair<Key, Value>> e_;   // oldest first
};

// The device copies of one kind of table that a context keeps, least recently used out.  An entry with an empty buffer is a
// negative one ("this key has no table"): it takes a place like any other, so that a stream of such a key does not ask the
// builder at every launch.
// Launches that read an evicted copy may still be queued on any stream or lane of the context, so making room waits for the
// whole device before the copy is freed.
template <typename Key, typename T, size_t CAPACITY>
class DevTableLru {
public:
    // the entry of `key`, now the most recently used; nullptr: none
    const DevTable<T> *find(const Key &key)
    {
        for (auto it = e_.begin(); it != e_.end(); ++it)
            if (same_bits(it->key, key)) {
                std::rotate(it, it + 1, e_.end());
                return &e_.back().d;
            }
        return nullptr;
    }
    // a free place for the next insert; on its own before the newcomer is allocated, where one table too many might not fit
    hipError_t make_room()
    {
        if (e_.size() < CAPACITY)
            return hipSuccess;
        const hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess)
            e_.erase(e_.begin());
        return e;
    }
    hipError_t insert(const Key &key, DevTable<T> d)
    {
        const hipError_t e = make_room();
        if (e == hipSuccess)
            e_.push_back({key, std::move(d)});
        return e;
    }
    int resident() const   // entries with a device copy
    {
        return (int)std::count_if(e_.begin(), e_.end(), [](const Entry &e) { return (bool)e.d; });
    }
    void clear() { e_.clear(); }

private:
    struct Entry {
        Key key;
        DevTable<T> d;
    };
    std::vector<Entry> e_;   // least recently used first
};

}  // namespace lhost

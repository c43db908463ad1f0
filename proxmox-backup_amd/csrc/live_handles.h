// The handles of one type that are alive: every job's C ABI (garbage collection, verify, sync,
// backup; device side and host mirror alike) checks a handle against this registry before it
// touches it, adds it in begin and removes it in end.  Plain C++.
#pragma once
#include <mutex>
#include <set>

namespace pbs {

template <class H>
struct Live {
    std::mutex mu;
    std::set<const H*> handles;
    static Live& get() {
        static Live* l = new Live;  // never destroyed
        return *l;
    }
    static bool alive(const H* h) {
        if (!h) return false;
        Live& l = get();
        std::lock_guard<std::mutex> g(l.mu);
        return l.handles.count(h) != 0;
    }
    static void add(const H* h) {
        Live& l = get();
        std::lock_guard<std::mutex> g(l.mu);
        l.handles.insert(h);
    }
    static bool remove(const H* h) {
        Live& l = get();
        std::lock_guard<std::mutex> g(l.mu);
        return l.handles.erase(h) != 0;
    }
};

}  // namespace pbs

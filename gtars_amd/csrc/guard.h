// guard.h -- the error status, the exception guard and the malloc'ed result array of the C entry points, for the HIP
// translation units (through common.h) and the plain C++ host layers alike: no HIP headers here.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <exception>
#include <new>
#include <string>

#include "../../include/gtars_amd.h"

namespace gtars {

// records msg as the calling thread's last error and returns st (api.hip)
gtars_status fail(gtars_status st, const std::string &msg);

// runs f(), turning C++ exceptions into a status (nothing may unwind through the extern "C" boundary)
template <class F>
inline gtars_status guarded(F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return fail(GTARS_ERR_INTERNAL, "out of host memory");
    } catch (const std::exception &e) {
        return fail(GTARS_ERR_INTERNAL, std::string("internal error: ") + e.what());
    }
}

// an array that a C entry point hands to its caller (gtars_free): malloc'ed, freed here unless release()d
template <class T>
struct MallocArray {
    T *p = nullptr;
    ~MallocArray() { free(p); }
    bool alloc(uint64_t n) {
        p = (T *)malloc((n ? n : 1) * sizeof(T));
        return p != nullptr;
    }
    T *release() {
        T *r = p;
        p = nullptr;
        return r;
    }
};

}  // namespace gtars

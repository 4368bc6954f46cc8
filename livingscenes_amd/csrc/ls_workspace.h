// ls_workspace.h -- the one statement of how an operator's caller-provided workspace is cut up: pieces that start on multiples of
// kWorkspaceAlign bytes, one after another from the base.  Every operator has ONE layout function that takes its pieces from an Arena; the
// ls_<op>_workspace_bytes() query runs it over a null base (a sizing pass: every pointer null, bytes() the size) and the entry point over the
// caller's workspace, so the size the query reports and the bytes the operator touches cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

namespace ls {

constexpr size_t kWorkspaceAlign = 256;
__host__ __device__ inline size_t align256(size_t x) { return (x + kWorkspaceAlign - 1) & ~(kWorkspaceAlign - 1); }

class Arena {   // host only
    char* base_;
    size_t end_ = 0;
public:
    explicit Arena(void* base) : base_((char*)base) {}   // nullptr: a sizing pass
    // the next piece as an offset from the base, for plans that store offsets
    size_t take_bytes(size_t bytes) {
        const size_t o = align256(end_);
        end_ = o + bytes;
        return o;
    }
    template <class T>
    T* take(size_t count) {
        const size_t o = take_bytes(count * sizeof(T));
        return base_ ? (T*)(base_ + o) : nullptr;
    }
    size_t bytes() const { return align256(end_); }   // the total so far, a multiple of kWorkspaceAlign
    // ... without the padding after the last piece: only for the two sizes that have always ended there (match.hip, the encoder tail)
    size_t bytes_unpadded() const { return end_; }
};

}  // namespace ls

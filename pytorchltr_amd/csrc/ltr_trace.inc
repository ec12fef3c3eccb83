// ltr_trace.inc -- the trace stamps of the fused Linear scorer + loss kernels, in ONE place.  In the product build (no
// -DLTR_TRACE) every macro below expands to nothing: the kernels carry no stamp and no extra argument.  Trace builds
// (scripts/build_variants.sh name:"-DLTR_TRACE -DLTR_TRACE_WALL", scripts/trace_regtile.py, scripts/cu_bytes.py) write
// per-workgroup time stamps and the placement (HW_ID / XCC_ID) into the buffer passed as `scores_out`.
#ifdef LTR_TRACE
// -DLTR_TRACE_WALL: stamps from the 100 MHz constant clock (comparable across CUs / XCDs)
#ifdef LTR_TRACE_WALL
#define LTR_NOW() ((long long)wall_clock64())
#else
#define LTR_NOW() ((long long)__builtin_readcyclecounter())
#endif
#define LTR_STAMP(i) do { if (tid == 0 && p.scores_out) reinterpret_cast<long long *>(p.scores_out)[(size_t)b * 8 + (i)] = LTR_NOW(); } while (0)
#define LTR_STAMP2(i) do { if (tid == 0 && p.scores_out) reinterpret_cast<long long *>(p.scores_out)[(size_t)b * 16 + (i)] = LTR_NOW(); } while (0)
#define LTR_TRACE_ENTRY() const long long t_entry = LTR_NOW()
// slot 14: the workgroup's entry time; slot 15: block id | HW_ID << 32 | XCC_ID << 48
#define LTR_TRACE_PLACEMENT()                                                                                          \
    do {                                                                                                               \
        if (tid == 0 && p.scores_out) {                                                                                \
            unsigned hwid_, xcc_;                                                                                      \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid_));                                        \
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));                                        \
            reinterpret_cast<long long *>(p.scores_out)[(size_t)b * 16 + 14] = t_entry;                                \
            reinterpret_cast<long long *>(p.scores_out)[(size_t)b * 16 + 15] =                                         \
                (long long)blockIdx.x | ((long long)(hwid_ & 0xffff) << 32) | ((long long)(xcc_ & 0xf) << 48);         \
        }                                                                                                              \
    } while (0)
// the lazy launch (scripts/trace_regtile.py --lazy): slot 7 the tile burst issued, slot 11 the weights received from the granules;
// a reducer workgroup stamps row B + its block id -- slot 0 its entry, slot 1 its granules stored.  The lazy step's entry points
// take no score matrix: the buffer comes from ltr_debug_trace_buffer (B + reducers rows of 16 words; null: an untraced launch).
#define LTR_TRACE_REDUCER(i) do { if (threadIdx.x == 0 && p.scores_out) reinterpret_cast<long long *>(p.scores_out)[((size_t)p.B + blockIdx.x) * 16 + (i)] = LTR_NOW(); } while (0)
inline float *&trace_buffer() { static float *v = nullptr; return v; }
#define LTR_TRACE_BUFFER(scores_out) ((scores_out) ? (scores_out) : trace_buffer())
// the pair pass's own stamps (slots 8 .. 10): extra trailing arguments of pairwise_core_sym
#define LTR_SYM_TRACE_ARGS , 0, 1, false, (p.scores_out ? reinterpret_cast<long long *>(p.scores_out) + (size_t)b * 16 + 8 : nullptr)
#define LTR_TRACE_ALLOW_FAST(scores_out) true          /* tuning build: scores_out is the trace buffer */
#else
#define LTR_STAMP(i) do { } while (0)
#define LTR_STAMP2(i) do { } while (0)
#define LTR_TRACE_ENTRY() do { } while (0)
#define LTR_TRACE_PLACEMENT() do { } while (0)
#define LTR_TRACE_REDUCER(i) do { } while (0)
#define LTR_TRACE_BUFFER(scores_out) (scores_out)
#define LTR_SYM_TRACE_ARGS
#define LTR_TRACE_ALLOW_FAST(scores_out) ((scores_out) == nullptr)
#endif

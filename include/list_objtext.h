/*
 * list_objtext.h -- C ABI of the Wavefront .obj writer for predicted meshes on the MI355X (gfx950): the text of the
 * file utils.write_obj writes, composed on the device from the vertex and face tensors where list_mc_emit,
 * list_cc_compact or list_simp_emit left them.  The reference writes the file line by line on the host.  Exported from
 * the same liblist_hip.so as include/list_hip.h.
 *
 * Conventions: those of list_simplify.h (raw device pointers, caller-owned output and workspace, work enqueued on the
 * caller's stream, no allocation and no synchronisation inside, LIST_OK or a negative ListStatus); the description of
 * a failure is read with list_objtext_last_error() (thread-local).  list_objtext_host takes HOST pointers and uses no
 * device.
 *
 * ---- the rule -------------------------------------------------------------------------------------------------------
 * Inputs.  verts float32 [V][3], faces int32 [F][3], 0 <= V, F and V + F < INT32_MAX.  All vertex lines come first, then
 * all face lines; every line ends in '\n'.
 *   vertex (x, y, z)   "v " s(x) " " s(y) " " s(z) "\n"
 *   face (a, b, c)     "f " d(a+1) " " d(b+1) " " d(c+1) "\n"
 * d is the decimal of the index plus one computed in int64, with a leading '-' when negative.  No index is validated.
 * (utils.write_obj adds the one in int32, which overflows for a = INT32_MAX alone; this header prints 2147483648 there.)
 * s is what the f-string of utils.write_obj makes of a numpy.float32: format(x, "") hands the value to Python's float, so
 * the text is repr(float(x)), the shortest digits of the value WIDENED to float64 (0.1f prints 0.10000000149011612).
 * Computed from the bit pattern alone, in integer arithmetic:
 *   - a NaN of either sign and any payload is "nan"; infinities are "inf" and "-inf"; zeros are "0.0" and "-0.0";
 *   - digits: the shortest decimal digit string d1..dn (1 <= n <= 17) with an exponent that lies in the rounding interval
 *     of the float64.  The interval ends at the midpoints to the neighbouring float64s (the lower half is half as wide
 *     when x is a power of two) and its ends are included, as the widened significand is always even.  Among the
 *     shortest, the one closest to the value (Ryu's float64 rule);
 *   - layout, on the digits: with x = d1.d2..dn * 10^e, -4 <= e < 16 is positional, with at least one digit on each side
 *     of the point, zeros up to the point and then ".0" (0.5, 16777216.0, 9999999198822400.0, 0.00010000000474974513);
 *     anything else is d1[.d2..dn]e+XX or e-XX with two exponent digits (9.999999747378752e-05, 1.401298464324817e-45,
 *     1.0000000272564224e+16).
 * A token is at most 23 bytes, a vertex line at most 74, a face line at most 38.
 *
 * ---- call sequence --------------------------------------------------------------------------------------------------
 *   bytes = list_objtext_workspace_bytes(V, F);                         (0: refused, see list_objtext_last_error)
 *   list_objtext_count(verts, faces, V, F, ws, bytes, totals, stream);
 *   copy totals (DEVICE int64[2] = {bytes of the file, bytes of its vertex lines}) to the host, allocate out;
 *   list_objtext_emit(verts, faces, V, F, ws, bytes, out, n_out_bytes, stream);
 *
 * list_objtext_count leaves every line's byte offset (int64) in the workspace, which list_objtext_emit reads: the same
 * workspace, untouched in between, and the same verts, faces, V and F.  out may start at any byte address.  A byte at or
 * past n_out_bytes is skipped, never written.  V = 0 and F = 0 are valid (a point cloud is F = 0); with both 0 every
 * call returns LIST_OK and the totals are 0.  No atomics; no thread waits for another.
 *
 * list_objtext_host writes the same bytes on the host, from the same source compiled for the CPU: at most `cap` bytes go
 * to out (which may be NULL when cap is 0), and the file's full length is returned, or a negative ListStatus.
 */
#ifndef LIST_OBJTEXT_H
#define LIST_OBJTEXT_H

#include <stddef.h>
#include <stdint.h>

#include "list_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LIST_OBJTEXT_MAX_TOKEN 23
#define LIST_OBJTEXT_MAX_VERTEX_LINE 74
#define LIST_OBJTEXT_MAX_FACE_LINE 38
#define LIST_OBJTEXT_N_TOTALS 2

size_t list_objtext_workspace_bytes(int64_t V, int64_t F);
int list_objtext_count(const float* verts, const int32_t* faces, int64_t V, int64_t F, void* workspace,
                       size_t workspace_bytes, int64_t* totals, void* stream);
int list_objtext_emit(const float* verts, const int32_t* faces, int64_t V, int64_t F, const void* workspace,
                      size_t workspace_bytes, uint8_t* out, int64_t n_out_bytes, void* stream);
int64_t list_objtext_host(const float* verts, const int32_t* faces, int64_t V, int64_t F, uint8_t* out, int64_t cap);
const char* list_objtext_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* LIST_OBJTEXT_H */

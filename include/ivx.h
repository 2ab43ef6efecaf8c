/*
 * ivx.h -- C ABI of libivx.so: the MI355X (gfx950) implementation of the InVesalius dense-voxel
 * hot path (threshold / region growing / watershed masks, MIP-family projections, marching cubes)
 * and of the stages SURVEY.md 8(f) ranks next to it (indexed surface, largest region, area / volume,
 * context-aware smoothing, view-matrix resampling, 3-D mask editing, mask measurements).
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain pointers, sizes and
 * byte strides (no torch / numpy / VTK types) and returns an int status (IVX_OK or a negative
 * IVX_E* code; ivx_last_error() gives the text).  Each declaration cites the reference interface it
 * replaces (paths relative to the invesalius3 checkout).  INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add; invesalius3_amd/ is that stub, complete.
 *
 * Two layers:
 *   ivx_dev_*   operate on DEVICE pointers (dense C-order [z][y][x] arrays already resident in HBM)
 *               on a caller-supplied HIP stream (void* == hipStream_t, NULL = default stream).
 *               Used by the resident pipeline (bench.py, the multi-GPU slab driver).
 *   ivx_*       operate on HOST pointers with byte strides (numpy arrays / np.memmap views such as
 *               mask.matrix[1:,1:,1:]); they stage through HBM, run the same kernels and write the
 *               result in place into the caller-owned output, exactly like the PyO3 functions.
 *
 * There is NO CPU fallback anywhere in this library: without a HIP device every compute entry
 * point returns IVX_EHIP.
 *
 * Conventions (identical to the reference): arrays are [z][y][x]; seeds are (x,y,z);
 * axis 0/1/2 = AXIAL/CORONAL/SAGITAL = reduce over z/y/x; strct is the 3x3x3 (or 1x3x3 ...) uint8
 * structuring element from scipy.ndimage.generate_binary_structure.
 */
#ifndef IVX_H
#define IVX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVX_OK 0
#define IVX_EINVAL (-1) /* bad dtype / shape / argument        -> Python TypeError / ValueError   */
#define IVX_ERANGE (-2) /* seed or label out of bounds          -> IndexError (Rust: index panic)  */
#define IVX_ENOMEM (-3) /* host or device allocation failed     -> MemoryError                     */
#define IVX_EDOM (-4)   /* NumCast failure                      -> ValueError (Rust: unwrap panic) */
#define IVX_EHIP (-5)   /* HIP runtime error / no device        -> RuntimeError                    */
#define IVX_ESTALE (-6) /* a registered host array was written without ivx_host_touch (only with the stale check on) */
#define IVX_EINTERNAL (-7) /* a bounded device loop ran to its bound: a defect of the library -> RuntimeError */

/* dtype codes (image dtypes accepted by the reference's ImageTypes3 enum, invesalius_rs/src/types.rs:4-70) */
#define IVX_U8 0
#define IVX_I16 1
#define IVX_F64 2
#define IVX_U16 3
#define IVX_F32 4 /* mesh vertices */
#define IVX_I32 5 /* label volumes (LabelsTypes3) */
#define IVX_I64 6
#define IVX_I8 7 /* watershed markers (watershed_process.py:57 casts to int8) */

/* projection ops for ivx_*mip_reduce (numpy .max/.min/.mean, invesalius/data/slice_.py:885-889) */
#define IVX_MIP_MAX 0
#define IVX_MIP_MIN 1
#define IVX_MIP_MEAN 2
#define IVX_MIP_SUM 3 /* exact int64 sums: what a Z-sharded MeanIP all-reduces before dividing */

/* ------------------------------------------------------------------------------------------------
 * runtime
 * ---------------------------------------------------------------------------------------------- */
int ivx_version(void);
const char *ivx_last_error(void);
int ivx_device_count(int *count);
int ivx_set_device(int device);
int ivx_device_synchronize(void);
int ivx_device_name(char *buf, size_t buflen);
int ivx_malloc(void **dptr, size_t nbytes);
int ivx_free(void *dptr);
int ivx_memset(void *dptr, int value, size_t nbytes, void *stream);
int ivx_memcpy_h2d(void *dst, const void *src, size_t nbytes);
int ivx_memcpy_d2h(void *dst, const void *src, size_t nbytes);
int ivx_memcpy_d2d(void *dst, const void *src, size_t nbytes, void *stream);
/* the sharded flood's vote words (invesalius3_amd/parallel.py, slab_region_grow; no counterpart upstream -- the reference has no
 * multi-GPU code): votes[0] = what ivx_comm_exchange_vote all-reduces, votes[1] = the words this rank's last OR gained.
 * _set: both words by a one-thread kernel; _read: both words to the host through the pinned mailbox (no stream
 * synchronisation), after which votes[0] <- votes[1] and votes[1] <- 0 on the device -- staged for the next round's all-reduce and
 * for ivx_dev_flood_or_planes_acc */
int ivx_dev_vote_set(int32_t *votes, int32_t v0, int32_t v1, void *stream);
int ivx_dev_vote_read(int32_t *votes, int32_t out[2], void *stream);
/* page-locked host memory (hipHostMalloc): arrays kept there cross PCIe at the link's rate instead of through the runtime's
 * bounce buffers; every host pointer of this header may point into it */
int ivx_host_alloc(void **hptr, size_t nbytes);
int ivx_host_free(void *hptr);
int ivx_stream_create(void **stream);
int ivx_stream_create_low_priority(void **stream); /* yields to default-priority streams when both have work */
int ivx_stream_destroy(void *stream);
int ivx_stream_synchronize(void *stream);
/* HIP events on the stream the kernels are launched on (bench.py roofline timing) */
int ivx_event_create(void **event);
int ivx_event_create_sync(void **event); /* for ordering streams (record + ivx_stream_wait_event), not for timing */
int ivx_event_destroy(void *event);
int ivx_event_record(void *event, void *stream);
int ivx_stream_wait_event(void *stream, void *event); /* work queued on `stream` after this call waits for `event` */
int ivx_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on `stop` */
/* free the cached device workspaces the host-level entry points keep between calls */
int ivx_release_workspace(void);

/* ------------------------------------------------------------------------------------------------
 * resident host arrays: the project's image and mask matrices stay in HBM between host-level calls
 *   no counterpart upstream: the reference keeps one array per project (`Slice.matrix`,
 *   invesalius/data/slice_.py:175-188; `Mask.matrix`, invesalius/data/mask.py:422-431) and hands it to the
 *   native layer again and again (styles.py:3200-3203, slice_.py:898,906); the host-level entry points of
 *   this header keep that call surface, so without this block each of them stages its inputs per call.
 * ivx_host_register mirrors the byte range [base, base + nbytes) on the current device, uploads it once and
 * returns a handle.  From then on every host-level entry point of this header (and ivx_memcpy_h2d / _d2h,
 * ivx_upload_strided / ivx_download_strided) that is handed memory whose whole byte extent -- computed from
 * shape and signed byte strides -- lies inside the range
 *   - takes its input from the mirror, device to device (dense, re-pitched, or gathered element by element for
 *     short rows, stepped, reversed and transposed views) instead of from the host;
 *   - writes its output to the host as before (the host copy is the authoritative one) AND into the mirror.
 * A library write that only partly overlaps a range marks the overlap stale; it is uploaded again at the next
 * use.  The calls stay synchronous: the destination is complete on return.
 * The host side of the bargain: whoever writes registered memory with the CPU says so with ivx_host_touch /
 * ivx_host_touch_range (offset and size in bytes from `base`); exactly those bytes are uploaded again at the
 * next use.  ivx_host_set_check(1) (or IVX_RESIDENT_CHECK=1) makes every use compare the host bytes with the
 * mirror first and fail with IVX_ESTALE -- ivx_last_error() names the first differing byte offset -- at the
 * price of the upload the registration saves: a debugging aid, off by default.
 * Rules: overlapping registrations are IVX_EINVAL; a view with a zero stride on an axis longer than 1 counts as
 * not registered; a mirror belongs to the device that was current at registration, on any other device the
 * range counts as not registered; a handle is a generation number that is never given out twice, so a released
 * handle is IVX_EINVAL, never a lookup by address; ivx_host_release waits for a copy that is using the mirror.
 * A mirror that does not fit is IVX_ENOMEM and the range stays unregistered (no eviction).  With nothing
 * registered no byte moves differently.
 * ivx_host_stats: out = { uploads served, bytes served, refresh uploads, bytes re-uploaded, write-throughs,
 * bytes written through, invalidations, generation }.  ivx_transfer_stats (process-wide): out = { bytes the
 * copy helpers moved host -> device, device -> host, host -> device for the stale check alone (not in [0]),
 * bytes served from mirrors }.  Only the copy helpers named above are counted -- what carries images, masks and
 * their views, the offset table of a packed refresh included; small arguments that an entry point sends with a
 * plain hipMemcpy (seeds, the per-slice skip flags of ivx_threshold_all_slices, mesh arrays) are not.
 * ---------------------------------------------------------------------------------------------- */
int ivx_host_register(const void *base, size_t nbytes, uint64_t *handle);
int ivx_host_touch(uint64_t handle);
int ivx_host_touch_range(uint64_t handle, size_t offset, size_t nbytes);
int ivx_host_release(uint64_t handle);
int ivx_host_stats(uint64_t handle, uint64_t out[8]);
int ivx_host_count(uint64_t *count); /* live registrations */
int ivx_host_set_check(int on);
int ivx_transfer_stats(uint64_t out[4]);
/* a 3-D host view (signed byte strides, itemsize 1 / 2 / 4 / 8) <-> a dense device block: the staging every host-level
 * entry point does with its arrays, for callers that keep device blocks of their own (DeviceBuffer.upload_view) */
int ivx_upload_strided(void *dst, const void *src, const int64_t shape[3], const int64_t strides[3], size_t itemsize);
int ivx_download_strided(void *dst, const int64_t shape[3], const int64_t strides[3], const void *src, size_t itemsize);

/* ------------------------------------------------------------------------------------------------
 * threshold -> uint8 mask
 *   replaces Slice.do_threshold_to_a_slice / do_threshold_to_all_slices
 *            invesalius/data/slice_.py:1722-1737, 1739-1769            (preserve = 1)
 *        and Slice.SetMaskThreshold whole-volume loop slice_.py:1240-1247 (preserve = 0)
 * mask[v] = (lo <= img[v] <= hi) ? 255 : 0; with preserve, existing 1/2/253/254 are kept.
 * skip_flags (dz bytes, may be NULL): slices with a non-zero flag are left untouched
 * (mask.matrix[n,0,0] != 0 test, slice_.py:1761).
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_threshold_i16(const int16_t *img, int64_t dz, int64_t dy, int64_t dx, int lo, int hi,
                          int preserve, const uint8_t *skip_flags, uint8_t *mask, void *stream);
/* threshold (no preserve rule, no skip flags) that also emits the mask's inside-bit plane (mask >= 127), in the
 * layout of the region-growing / marching-cubes planes (64 x-voxels per uint64).  Needs dx % 64 == 0 and 16-byte
 * aligned buffers (IVX_EINVAL otherwise: use ivx_dev_threshold_i16).  bits: dz*dy*(dx/64) words. */
int ivx_dev_threshold_i16_bits(const int16_t *img, int64_t dz, int64_t dy, int64_t dx, int lo, int hi, uint8_t *mask,
                               uint64_t *bits, void *stream);
/* Per-word (min, max) records of an int16 image: one uint32 per plane word (64 x-voxels, index (z*dy + y)*(dx/64) + x/64 like
 * the bit planes), min as int16 in the low half, max as int16 in the high half.  A word wholly inside or wholly outside
 * [lo, hi] is thresholded from its record alone.  Only for dx % 64 == 0 (IVX_EINVAL otherwise).
 *   ivx_image_ranges_bytes: size of the record buffer.
 *   ivx_dev_image_ranges_i16: build the records in one pass over the image.
 *   ivx_dev_threshold_i16_bits_ranges: ivx_dev_threshold_i16_bits with the records;
 *     mode IVX_RANGES_BUILD writes them as a by-product of the pass (the first threshold after the image's bytes changed),
 *     mode IVX_RANGES_USE reads them and loads voxels of mixed words only (every later threshold of the same image).
 *   Mask and plane are byte for byte those of ivx_dev_threshold_i16_bits in both modes, for every lo / hi -- PROVIDED the
 *   records describe the image: use mode trusts them and does not look at a word they decide.  Whoever writes the image
 *   must rebuild (or build-mode again) before the next use-mode call. */
#define IVX_RANGES_BUILD 0
#define IVX_RANGES_USE 1
int ivx_image_ranges_bytes(int64_t dz, int64_t dy, int64_t dx, size_t *nbytes);
int ivx_dev_image_ranges_i16(const int16_t *img, int64_t dz, int64_t dy, int64_t dx, uint32_t *ranges, void *stream);
int ivx_dev_threshold_i16_bits_ranges(const int16_t *img, int64_t dz, int64_t dy, int64_t dx, int lo, int hi,
                                      uint8_t *mask, uint64_t *bits, uint32_t *ranges, int mode, void *stream);
/* The plane-only forms of ivx_dev_threshold_i16_bits and ivx_dev_threshold_i16_bits_ranges: the same plane (and, in build
 * mode, the same records), no mask.  For a caller that keeps "mask == 255 * plane" as a note and has the bytes written later,
 * by ivx_dev_mask_from_planes.  Same argument rules without `mask`. */
int ivx_dev_threshold_i16_plane(const int16_t *img, int64_t dz, int64_t dy, int64_t dx, int lo, int hi, uint64_t *bits,
                                void *stream);
int ivx_dev_threshold_i16_plane_ranges(const int16_t *img, int64_t dz, int64_t dy, int64_t dx, int lo, int hi, uint64_t *bits,
                                       uint32_t *ranges, int mode, void *stream);
/* Host form. `mask` points at the FULL (dz+1,dy+1,dx+1) matrix of invesalius/data/mask.py:422-431
 * (flag cells in the index-0 planes); strides in bytes.  With honour_flags the per-slice flag
 * mask[n,0,0] is tested and then set to 1 (slice_.py:1761-1767); without it every slice is
 * processed and the flag forced to 1 (slice_.py:1240-1247). */
int ivx_threshold_all_slices(const int16_t *img, const int64_t shape[3], const int64_t img_strides[3],
                             int lo, int hi, int preserve, int honour_flags, uint8_t *mask,
                             const int64_t mask_strides[3]);

/* ------------------------------------------------------------------------------------------------
 * MaxIP / MinIP / MeanIP along an axis
 *   replaces numpy .max/.min/.mean(axis) in Slice.get_image_slice slice_.py:885-889,969-973,1056-1060
 * out is 2-D: axis0 -> (dy,dx), axis1 -> (dz,dx), axis2 -> (dz,dy); dtype == image dtype for
 * max/min, float64 for mean (numpy semantics).
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_mip_reduce(int dtype, const void *vol, int64_t dz, int64_t dy, int64_t dx, int axis, int op,
                       void *out, void *stream);
int ivx_mip_reduce(int dtype, const void *vol, const int64_t shape[3], const int64_t strides[3], int axis,
                   int op, void *out, const int64_t out_strides[2]);
/* viewport magnification of a projection: dst (h*f, w*f) = every pixel of src (h, w) repeated f x f times -- what the
 * reference's ray caster renders for axis-aligned rays at SetImageSampleDistance(1/f) (invesalius/data/volume.py:678) */
int ivx_dev_replicate_i16(const int16_t *src, int64_t h, int64_t w, int factor, int16_t *dst, void *stream);

/* ------------------------------------------------------------------------------------------------
 * MIDA, LMIP, fast contour MIP
 *   replaces mida / lmip / fast_countour_mip of invesalius_rs/src/mips.rs:7-279
 *   (bindings mips_py.rs:161-253, wrappers invesalius_rs/__init__.py:91-101)
 * dtype pairs (in -> out): i16->i16, u8->u8, f64->u8 for mida; out dtype == in dtype otherwise.
 * A NumCast failure on any output pixel returns IVX_EDOM (the reference panics).
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_minmax_f32(int dtype, const void *vol, int64_t n, float *minmax2, void *stream);
int ivx_dev_mida(int dtype, const void *vol, int64_t dz, int64_t dy, int64_t dx, int axis, float wl, float ww,
                 const float *minmax2 /* device, from ivx_dev_minmax_f32 */, int out_dtype, void *out,
                 int *status /* device int, set to IVX_EDOM on cast failure */, void *stream);
int ivx_dev_lmip(int dtype, const void *vol, int64_t dz, int64_t dy, int64_t dx, int axis, double tmin,
                 double tmax, void *out, void *stream);
/* Z-sharded volumes, rays along Z: one slab's share of every ray.  state = 5 doubles per output pixel
 * (dy*dx*5), NULL state_in on the first slab, NULL state_out on the last one (which writes `out`).  kind 0 = LMIP
 * (p0, p1 = tmin, tmax), 1 = MIDA (p0, p1 = wl, ww; minmax2 = min / max of the WHOLE volume, device float32[2]). */
int ivx_dev_rays_z_slab(int kind, int dtype, const void *vol, int64_t dz, int64_t dy, int64_t dx, double p0, double p1,
                        const float *minmax2, const double *state_in, double *state_out, int out_dtype, void *out,
                        int *status, void *stream);
/* The contour volume of fast_countour_mip (calc_fcm_intensity, invesalius_rs/src/mips.rs:197-213).  `base^n` is Rust's f32::powf =
 * the platform libm's powf: reproduced bit for bit for glibc (csrc/glibc_powf.h restates its algorithm and tables; checked
 * against libm on 1.5e9 inputs) in the build this machine's glibc selects -- ivx_powf_variant(): 1 = the FMA build x86-64 glibc
 * runs on CPUs with FMA + AVX2, 0 = the plain build (override: IVX_POWF_VARIANT=fma|plain). */
int ivx_powf_variant(void);
/* out[i] = powf(x[i], y[i]) as the contour MIP computes it (device float arrays; variant 1 / 0 as above, -1 = this machine's).
 * Probes of the fused MaxIP's fast power (tests): 2 / 3 = its value and its relative bound. */
int ivx_dev_powf(const float *x, const float *y, float *out, int64_t n, int variant, void *stream);
/* (tests) the bounds the fused contour MaxIP folds for one voxel: d = the wrapped int16 difference along the ray, other = the two
 * across it (int16 pair in a word), n = the exponent in [1, 64]; the reference's float32 value must lie in [lo, hi]. */
int ivx_dev_fcm_bounds(const int32_t *d, const uint32_t *other, float n, float *lo, float *hi, int64_t count, void *stream);
int ivx_dev_fcm_volume(int dtype, const void *vol, int64_t dz, int64_t dy, int64_t dx, float n, int axis,
                       void *tmp /* same dtype/shape */, int *status, void *stream);
/* fast_countour_mip_internal with tmip == 0 (invesalius_rs/src/mips.rs:237-247: tmp = contour volume, out = fold_axis max):
 * the contour value is folded into the running maximum as it is computed -- no temp volume -- for int16 rows of whole
 * 16-byte chunks; other inputs materialise the volume in this stream's workspace.  int16 / uint8 images; `out` has the
 * image's dtype and the shape of the projection; *status receives IVX_EDOM where the reference's NumCast would panic. */
int ivx_dev_fcm_maxip(int dtype, const void *vol, int64_t dz, int64_t dy, int64_t dx, float n, int axis, void *out,
                      int *status, void *stream);
int ivx_mida(int dtype, const void *img, const int64_t shape[3], const int64_t strides[3], int axis,
             double wl, double ww, int out_dtype, void *out, const int64_t out_strides[2]);
int ivx_lmip(int dtype, const void *img, const int64_t shape[3], const int64_t strides[3], int axis,
             double tmin, double tmax, void *out, const int64_t out_strides[2]);
int ivx_fast_countour_mip(int dtype, const void *img, const int64_t shape[3], const int64_t strides[3],
                          float n, int axis, double wl, double ww, int tmip, void *out,
                          const int64_t out_strides[2]);

/* ------------------------------------------------------------------------------------------------
 * marching cubes == geometry of create_surface_piece
 *   replaces pad_image + converters.to_vtk + vtkImageFlip + vtkContourFilter
 *            invesalius/data/surface_process.py:52-68,100-186; invesalius/data/converters.py:34-101
 * `a` is the piece (mask[roi+1,1:,1:] u8 or image[roi] i16), dense (nz,ny,nx).  The padding
 * (pad_xy, pad_bottom, pad_top, pad_value) and the Y flip are folded into the addressing, never
 * materialised.  Output: triangle soup, 9 float32 per triangle, in iso-major then (k,j,i) raster
 * order of the padded+flipped cell grid.  Two-call protocol: count, then emit into a buffer of at
 * least `count` triangles.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ivx_mc_params {
    int32_t dtype;      /* IVX_U8 / IVX_I16 / IVX_U16 */
    int32_t pad_xy;     /* 1: one pad voxel on both sides in y and x */
    int32_t pad_bottom; /* 1: one pad slice before z=0 */
    int32_t pad_top;    /* 1: one pad slice after the last */
    int32_t vtk_pz;     /* z padding reported to to_vtk (== pad_bottom when fill_border_holes) */
    int32_t niso;       /* 1 or 2 */
    int64_t nz, ny, nx; /* piece shape */
    int64_t roi_start;  /* first image slice of the piece */
    double pad_value;
    double spacing[3]; /* (sx, sy, sz) */
    double iso[2];
} ivx_mc_params;
/* scratch needed by count/emit for this piece (bytes); pass a device buffer of that size */
int ivx_dev_mc_scratch_bytes(const ivx_mc_params *p, size_t *nbytes);
/* host only, for tests: slice k, cell row j and word-in-row w of n cell-word ids (word id = (k * (NY-1) + j) * WC + w of the
 * padded cell grid), by the division-free arithmetic and the per-piece constants the count and list kernels use */
int ivx_mc_split_word_ids(const ivx_mc_params *p, const uint32_t *wid, size_t n, uint32_t *k, uint32_t *j, uint32_t *w);
/* classify + per-row-group triangle counts + scan; *ntris (host) receives the total.  Every count (this one, the _async and
 * the _bits forms) voids what the library remembered about the piece counted into `scratch` before: its inside plane, its
 * triangle list, its iso-0 / iso-1 split and its vertex split.  A later call that needs one of them and does not find it
 * returns IVX_EINVAL ("... must follow ..."): after a queue-only count of a two-iso piece, ivx_dev_mc_total comes before
 * ivx_dev_mc_indexed_emit. */
int ivx_dev_mc_count(const ivx_mc_params *p, const void *a, void *scratch, int64_t *ntris, void *stream);
/* Queue-only forms: nothing comes back to the host, so ivx_dev_mc_emit can be queued right behind them with the
 * CAPACITY of `tris` as max_tris (the emit kernel reads the real count, and the iso-0 / iso-1 split, on the device and
 * writes min(count, max_tris) triangles).  ivx_dev_mc_total then fetches the count: if it exceeds the capacity, grow the
 * buffer and call ivx_dev_mc_emit again. */
int ivx_dev_mc_count_async(const ivx_mc_params *p, const void *a, void *scratch, void *stream);
int ivx_dev_mc_count_bits_async(const ivx_mc_params *p, const uint64_t *inside_bits, void *scratch, void *stream);
int ivx_dev_mc_total(const ivx_mc_params *p, void *scratch, int64_t *ntris, void *stream);
/* ivx_dev_mc_total is ordered behind everything queued on `stream`: when it returns, so have a list and an emit queued in
 * front of it.  ivx_dev_mc_total_early gives the same number (and, for two iso-values, sets the same split) as soon as the
 * count's own scan has run: the scan of a one-iso count publishes the total to the host itself, so this form launches nothing
 * and does NOT wait for a list or an emit queued behind the count -- they may still be running when it returns.  The soup is
 * then complete in stream order only: synchronise the stream (or order the reader behind it) before reading `tris` from
 * elsewhere or freeing `tris`, `scratch` or the inside plane.  It may be called before or after the emit, and more than once.
 * Where the scan's word cannot be used (two iso-values, or 64 other messages have gone through the library's host mailbox
 * since the count was queued) it does what ivx_dev_mc_total does. */
int ivx_dev_mc_total_early(const ivx_mc_params *p, void *scratch, int64_t *ntris, void *stream);
/* same, from an inside plane (value >= iso[0]) the caller already holds; niso must be 1.  The plane is read IN PLACE by
 * this call and by the ivx_dev_mc_emit / ivx_dev_mc_indexed_* calls that follow on the same scratch: keep it unchanged
 * until they have run. */
int ivx_dev_mc_count_bits(const ivx_mc_params *p, const uint64_t *inside_bits, void *scratch, int64_t *ntris,
                          void *stream);
/* emit; must follow ivx_dev_mc_count with the same params/scratch */
int ivx_dev_mc_emit(const ivx_mc_params *p, const void *a, const void *scratch, float *tris, int64_t max_tris,
                    void *stream);
/* ivx_dev_mc_emit for a uint8 mask (from_binary) whose bytes are KNOWN: v_out outside the inside plane the count ran on
 * (ivx_dev_mc_count_bits), v_sel where `sel_bits` (same layout) has a bit, v_in elsewhere inside -- the state a resident
 * threshold + region growing leaves behind.  No voxel is read: which end of an edge is inside is in the case index, so a
 * triangle costs three bit look-ups instead of six byte gathers; same arithmetic on the same numbers, same soup. */
int ivx_dev_mc_emit_levels(const ivx_mc_params *p, const void *scratch, const uint64_t *sel_bits, double v_out, double v_in,
                           double v_sel, float *tris, int64_t max_tris, void *stream);
/* the list pass of ivx_dev_mc_emit on its own (it needs the counts, not the voxels): queue it early, on the stream the
 * emit will use; the emit that follows with max_tris <= this max_tris skips its own list pass */
int ivx_dev_mc_list(const ivx_mc_params *p, const void *scratch, int64_t max_tris, void *stream);
/* The host form in two halves that share the device work (replaces the count call + emit call of the form below, which upload the
 * piece and count twice): _begin uploads, counts and emits into the library's own output block and returns the count; _fetch,
 * which must be the NEXT host-level call of the process, copies the soup into the array the caller sized from it (IVX_EINVAL when
 * anything came in between: take ivx_marching_cubes then).  Same soup, same order, same bits.
 * Replaces vtkContourFilter::Update of create_surface_piece (invesalius/data/surface_process.py:172-186). */
int ivx_marching_cubes_begin(const ivx_mc_params *p, const void *a, const int64_t strides[3], int64_t *ntris);
int ivx_marching_cubes_fetch(float *tris, int64_t ntris);
/* Host form: strided piece in, soup out.  tris == NULL -> count only.  Returns count in *ntris. */
int ivx_marching_cubes(const ivx_mc_params *p, const void *a, const int64_t strides[3], float *tris,
                       int64_t max_tris, int64_t *ntris);

/* Cross-slab stitch on the device (replaces vtkAppendPolyData + vtkCleanPolyData of join_process_surface,
 * invesalius/data/surface_process.py:229-268, across Z-slabs).  Follows ivx_dev_mc_indexed_emit on the same params / scratch /
 * stream, one iso-value.  Rank r's top point plane and rank r+1's bottom point plane are the same voxels: the vertices both
 * pieces carry there are matched by edge identity (point word, kind, bit), never by float compares.
 *   1. ivx_dev_mc_stitch_top_sig   -> 32 bytes per point word of the top plane; send them to the rank above
 *   2. ivx_dev_mc_stitch_match     bottom plane vs the signature received from below (NULL on the lowest rank):
 *                                  vd[0] = nverts, vd[1] = copies this piece drops (device words); all-gather the pairs
 *   3. ivx_dev_mc_stitch_apply     faces -> global vertex ids in place, kept vertices -> verts_out (nverts - dropped of
 *                                  them, old order; global id of the first = sum over lower ranks of nverts - dropped) */
int ivx_dev_mc_stitch_sig_bytes(const ivx_mc_params *p, size_t *nbytes);
int ivx_dev_mc_stitch_top_sig(const ivx_mc_params *p, const void *scratch, void *sig, void *stream);
int ivx_dev_mc_stitch_match(const ivx_mc_params *p, const void *scratch, const void *nbr_sig, int64_t nverts, uint32_t *vd,
                            void *stream);
int ivx_dev_mc_stitch_apply(const ivx_mc_params *p, const void *scratch, const void *nbr_sig, const uint32_t *vd_all, int rank,
                            const float *verts, int64_t nverts, int32_t *faces, int64_t ntris, float *verts_out, void *stream);
/* ------------------------------------------------------------------------------------------------
 * indexed surface ("point merge"): unique vertices + int32 faces instead of a soup
 *   replaces vtkAppendPolyData + vtkCleanPolyData of join_process_surface
 *            invesalius/data/surface_process.py:229-268
 * A vertex is a grid edge that crosses the iso-surface, so ids come from popcount scans of the crossing bit planes
 * (no hashing, no sorting); verts[faces] is bit-identical to the soup of ivx_dev_mc_emit, in the same triangle
 * order.  Edges that cross exactly AT a grid point (the sample equals the iso-value) share that point's one vertex,
 * so coincident positions are merged exactly as an exact-arithmetic point merge would; faces that thereby collapse
 * (two equal ids) are kept, so the triangle count and order stay those of the soup.  Protocol: ivx_dev_mc_count -> ivx_dev_mc_indexed_count -> ivx_dev_mc_indexed_emit (same params/scratch).
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_mc_indexed_count(const ivx_mc_params *p, const void *a, const void *scratch, int64_t *nverts, void *stream);
int ivx_dev_mc_indexed_emit(const ivx_mc_params *p, const void *a, const void *scratch, float *verts, int64_t max_verts,
                            int32_t *faces, int64_t max_tris, void *stream);
/* The two calls above for a uint8 mask whose bytes are KNOWN -- `v_out` outside the inside plane handed to
 * ivx_dev_mc_count_bits (and as padding), `v_sel` where `sel_bits` has a bit, `v_in` elsewhere inside; v_out < iso < v_in,
 * v_sel -- as a resident pipeline knows them after its threshold and region growing (see ivx_dev_mc_emit_levels): neither
 * the strictly-inside plane nor a vertex reads a voxel.  Same vertices and faces, bit for bit. */
int ivx_dev_mc_indexed_count_levels(const ivx_mc_params *p, const void *scratch, int64_t *nverts, void *stream);
int ivx_dev_mc_indexed_emit_levels(const ivx_mc_params *p, const void *scratch, const uint64_t *sel_bits, double v_out,
                                   double v_in, double v_sel, float *verts, int64_t max_verts, int32_t *faces,
                                   int64_t max_tris, void *stream);
int ivx_marching_cubes_indexed(const ivx_mc_params *p, const void *a, const int64_t strides[3], float *verts,
                               int64_t max_verts, int32_t *faces, int64_t max_tris, int64_t *nverts, int64_t *ntris);

/* ------------------------------------------------------------------------------------------------
 * surface post-processing on the indexed mesh (join_process_surface, invesalius/data/surface_process.py)
 *   ivx_*_mesh_keep_largest     replaces vtkPolyDataConnectivityFilter + SetExtractionModeToLargestRegion
 *                               surface_process.py:376-391.  Regions = triangles connected through shared vertex
 *                               ids; the region with the most triangles is kept (the one whose first triangle comes
 *                               first wins a tie); kept triangles stay in order, vertices are compacted in order.
 *   ivx_*_mesh_mass_properties  replaces vtkMassProperties (GetVolume / GetSurfaceArea) surface_process.py:452-458.
 *                               out8 = {volume, area, vol_x, vol_y, vol_z, kx, ky, kz}; faces == NULL -> `verts` is a
 *                               soup (3 vertices per triangle).
 * Device forms take device pointers; sizes come back on the host.  out_verts/out_faces == NULL -> sizes only.
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_mesh_keep_largest(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, float *out_verts,
                              int64_t max_verts, int32_t *out_faces, int64_t max_tris, int64_t *out_nverts,
                              int64_t *out_ntris, int64_t *nregions, void *stream);
int ivx_dev_mesh_mass_properties(const float *verts, const int32_t *faces, int64_t ntris, double *out8, void *stream);
int ivx_mesh_keep_largest(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, float *out_verts,
                          int32_t *out_faces, int64_t *out_nverts, int64_t *out_ntris, int64_t *nregions);
int ivx_mesh_mass_properties(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, double *out8);
/* The last two filters of join_process_surface (invesalius/data/surface_process.py:396-435), host arrays in and out:
 *   ivx_mesh_fill_holes     replaces vtkFillHolesFilter + SetHoleSize(hole_size) (:396-416): every closed rim of boundary
 *                           edges whose bounding sphere (half the diagonal of the rim's bounding box) has a radius <= hole_size
 *                           is capped by a fan from its centroid -- ONE new point per hole (index nverts + hole), cap triangles
 *                           wound so that the patch continues the surface.  Rims ordered by their smallest directed edge
 *                           3 f + k, triangles inside a rim in walking order from that edge.
 *   ivx_mesh_point_normals  replaces vtkPolyDataNormals (:420-435: FeatureAngle, SplittingOn, AutoOrientNormalsOn,
 *                           ComputeCellNormalsOn): unit cell normals; corners joined across edges whose cell normals' dot
 *                           product exceeds cos_feature_angle form fans, a vertex's smallest fan keeps the point, the others get
 *                           copies appended in (vertex, fan) order; point normal = normalised sum of the fan's cell normals;
 *                           with auto_orient a surface whose signed volume is negative is turned inside out first.
 * Both are two-call: with NULL output arrays the sizes come back (*n_new_verts / *n_new_tris, *out_nverts); the second call
 * passes the capacities in through the same arguments.  PARITY UNPINNED vs VTK 9.3 (third party, not installable here). */
int ivx_mesh_fill_holes(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, double hole_size,
                        float *new_verts, int32_t *new_faces, int64_t *n_new_verts, int64_t *n_new_tris);
int ivx_mesh_point_normals(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, double cos_feature_angle,
                           int splitting, int auto_orient, float *out_verts, int32_t *out_faces, float *point_normals,
                           float *cell_normals /* may be NULL */, int64_t *out_nverts);
/* Surface visibility: "Remove non-visible faces" (pu.RemoveNonVisibleFaces / pu.HasNonVisibleFaces,
 * invesalius/data/polydata_utils.py:281-455: off-screen renders of the mesh + vtkSelectVisiblePoints) as a depth-only
 * software rasteriser.  A view is plain numbers, built on the host from the mesh's bounds
 * (polydata_utils.views_for_positions); the kernels use + - * / in float64 only:
 *   d = v - eye;  xe = (d.x r.x + d.y r.y) + d.z r.z  (ye with `up`, ze with `fwd`);
 *   xs = (xe / (ze tan_half aspect) + 1) 0.5 width;  ys = (ye / (ze tan_half) + 1) 0.5 height;
 *   zw = (zfar (ze - znear)) / (ze (zfar - znear)).   A vertex with ze <= 0 is behind the eye: its triangles draw nothing
 *   and the point is not visible (never the case for a view made from the bounds).
 *   ivx_*_mesh_bounds          {xmin, xmax, ymin, ymax, zmin, zmax} over ALL points (zeros for an empty mesh).
 *   ivx_*_mesh_depth_raster    float32 depth[height][width] of one view, cleared to 1.0; pixel centre (i + .5, j + .5) on or
 *                              inside a triangle (either winding, edge functions evaluated from the smaller vertex id) gets
 *                              the float32-rounded screen-barycentric zw, minimum kept.  `stages`: IVX_RASTER_* bits (the
 *                              three stages can be run, and timed, in separate calls on one stream, in this order).
 *   ivx_*_mesh_visible_points  flags[v] = 1 when any view sees point v: inside the viewport and
 *                              zw < depth[(int)ys][(int)xs] + 0.01 (vtkSelectVisiblePoints' default tolerance).
 *   ivx_*_mesh_select_points   keeps the triangles with ANY corner flagged (`invert`: any corner NOT flagged), in order, and
 *                              compacts the points they use, in order.  out_verts / out_faces == NULL -> sizes only.
 *   ivx_mesh_remove_nonvisible the whole tool on host arrays: flags over `views`, then the selection (remove_visible -> invert).
 * PARITY UNPINNED vs VTK's OpenGL rasteriser (third party, not installable here). */
typedef struct ivx_mesh_view {
    double eye[3], right[3], up[3], fwd[3]; /* orthonormal camera frame; fwd looks from the eye at the focal point */
    double znear, zfar;                     /* clipping range along fwd */
    double tan_half, aspect;                /* tan(view angle / 2), width / height */
    int32_t width, height;
} ivx_mesh_view;
#define IVX_RASTER_CLEAR 1 /* depth <- 1.0, queue of big triangles <- empty */
#define IVX_RASTER_SMALL 2 /* lane per triangle; boxes of more than IVX_RASTER_SMALL_BOX pixels are queued */
#define IVX_RASTER_BIG 4   /* workgroup per queued triangle */
#define IVX_RASTER_ALL 7
#define IVX_RASTER_SMALL_BOX 64
int ivx_dev_mesh_bounds(const float *verts, int64_t nverts, float *bounds6, void *stream);
int ivx_dev_mesh_depth_raster(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                              const ivx_mesh_view *view /* host */, int stages, float *depth, void *stream);
int ivx_dev_mesh_visible_points(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                                const ivx_mesh_view *views /* host */, int nviews, uint8_t *flags, void *stream);
int ivx_dev_mesh_select_points(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const uint8_t *flags,
                               int invert, float *out_verts, int64_t max_verts, int32_t *out_faces, int64_t max_tris,
                               int64_t *out_nverts, int64_t *out_ntris, void *stream);
int ivx_mesh_bounds(const float *verts, int64_t nverts, float *bounds6);
int ivx_mesh_depth_raster(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const ivx_mesh_view *view,
                          float *depth);
int ivx_mesh_visible_points(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                            const ivx_mesh_view *views, int nviews, uint8_t *flags);
int ivx_mesh_select_points(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const uint8_t *flags,
                           int invert, float *out_verts, int32_t *out_faces, int64_t *out_nverts, int64_t *out_ntris);
int ivx_mesh_remove_nonvisible(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                               const ivx_mesh_view *views, int nviews, int remove_visible, float *out_verts,
                               int32_t *out_faces, int64_t *out_nverts, int64_t *out_ntris);

/* Surface view: shaded pictures of up to IVX_SURFACE_MAX_LAYERS surfaces (Surface._show_surface, invesalius/data/surface.py:
 * 1061-1116: vtkPolyDataMapper + vtkActor with back-face culling, a colour, an opacity and an interpolation mode, under the
 * parallel-projection camera of viewer_volume.SetViewAngle), DESIGN 7n.  float64 + - * / (and sqrt in the shading) in one order:
 *   px = 2 parallel_scale / height;  d = v - focal;  a dot product is (d.x a.x + d.y a.y) + d.z a.z;
 *   X = (d.right) / px + 0.5 width;  Y = 0.5 height - (d.up) / px (row 0 is the top);  t = d.dir (smaller is nearer).
 *   ivx_dev_surface_raster   keys[height][width] of ONE surface: a front-facing triangle (area < 0 in (X, Y), edge functions
 *                            as for ivx_*_mesh_depth_raster) covers a centre when its three edge functions are <= 0; the key is
 *                            (ord(float32 t at the centre) << 32) | triangle index with ord(bits) = bits ^ 0x80000000 for a
 *                            non-negative float and ~bits for a negative one; the 64-bit unsigned minimum is kept (an empty
 *                            pixel holds all ones), so the buffer does not depend on the order the triangles arrive in.
 *                            `stages`: IVX_RASTER_* bits, as for ivx_dev_mesh_depth_raster.
 *   ivx_dev_surface_resolve  per pixel: the layers' fragments sorted by (ord depth, layer index), everything behind the first
 *                            opaque one dropped, the rest blended far to near over the background, one white headlight along
 *                            `dir` (ambient 0, diffuse 1, specular 0).  `rgba`: float32[height][width][4], or uint8 with out_u8
 *                            (floor(255 v + 0.5) clamped).  ids (may be NULL): int32[height][width][2] = (layer, triangle) of
 *                            the nearest fragment, -1 where empty; depth (may be NULL): its float32 t, +inf where empty.
 *   ivx_surface_render       the whole picture from host arrays (the layers' `keys` are ignored).
 * PARITY UNPINNED vs VTK's OpenGL renderer (third party, not installable here). */
typedef struct ivx_surface_camera {
    double focal[3], right[3], up[3], dir[3]; /* orthonormal frame; dir is the direction of projection */
    double parallel_scale;                    /* half the viewport's height in world units */
    int32_t width, height;
} ivx_surface_camera;
typedef struct ivx_surface_layer {
    const float *verts;
    int64_t nverts;
    const int32_t *faces;
    int64_t ntris;
    const float *normals; /* one unit normal per point, or NULL: shaded flat */
    const uint64_t *keys; /* width * height keys from ivx_dev_surface_raster */
    float rgb[3];
    float opacity; /* 1 - transparency */
} ivx_surface_layer;
#define IVX_SURFACE_MAX_LAYERS 8
#define IVX_SURFACE_FLAT 0
#define IVX_SURFACE_GOURAUD 1
#define IVX_SURFACE_PHONG 2
int ivx_dev_surface_raster(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris,
                           const ivx_surface_camera *cam /* host */, int stages, uint64_t *keys, void *stream);
int ivx_dev_surface_resolve(const ivx_surface_layer *layers /* host */, int nlayers, const ivx_surface_camera *cam /* host */,
                            int interpolation, const float *background /* 3 */, int out_u8, void *rgba, int32_t *ids, float *depth,
                            void *stream);
int ivx_surface_render(const ivx_surface_layer *layers, int nlayers, const ivx_surface_camera *cam, int interpolation,
                       const float *background, int out_u8, void *rgba, int32_t *ids, float *depth);

/* Surface connectivity tools beyond keep-largest (Surface.OnSplitSurface / OnSeedSurface, invesalius/data/surface.py:319-411;
 * pu.SplitDisconectedParts / pu.JoinSeedsParts, invesalius/data/polydata_utils.py:206-278: vtkPolyDataConnectivityFilter in its
 * SpecifiedRegions and PointSeededRegions modes), DESIGN 7h.  Regions are keep-largest's: triangles joined through shared point
 * ids.  Region r is the r-th region in ascending order of its first (smallest-index) triangle -- the `r` of AddSpecifiedRegion.
 *   ivx_*_mesh_region_labels  tri_labels[t] = region of triangle t; vert_labels[v] = region of point v, -1 when no triangle uses
 *                             it (either array may be NULL).
 *   ivx_*_mesh_split          every part at once: out_faces holds all ntris triangles grouped by region (original order inside
 *                             a region) with PART-LOCAL point ids, out_verts the used points grouped the same way (original
 *                             order inside a region), table[r] = {triangle offset, triangles, point offset, points} of part r.
 *                             Output arrays NULL -> sizes only (*out_nverts, *nparts); the host form takes the capacities of
 *                             out_verts / table in through *out_nverts / *nparts on the filling call (out_faces: ntris rows).
 *   ivx_*_mesh_parts_mass     out[8 r ..] = ivx_*_mesh_mass_properties' out8 of part r (its own cell count in the weights).
 *                             The number of launches does not depend on the number of parts.  small_max: parts of up to that
 *                             many triangles are reduced by one wave each, larger ones by the two-kernel path of
 *                             ivx_dev_mesh_mass_properties on their slice (<= 0: the default, 1024); `ntris` = all triangles.
 *   ivx_*_mesh_select_seeded  the union of the regions that hold a seed point, as triangles in order on their points compacted
 *                             in order.  Duplicate seeds are harmless, a seed no triangle uses selects nothing, no seeds give an
 *                             empty mesh.  Host form: a seed outside [0, nverts) is IVX_EDOM (DEVIATION: VTK skips negative ids
 *                             and reads past its array for large ones); the device form ignores such seeds.
 *   ivx_*_mesh_nearest_point  id of the point with the smallest squared distance to xyz (host doubles), computed in double as
 *                             (dx dx + dy dy) + dz dz; the smallest id on a tie; -1 for no points.
 *   ivx_dev_partition_u32     the stable many-way partition behind the split: order[] = item indices grouped by key (keys < nkeys,
 *                             original order inside a key), offsets[k] = items with a key below k (nkeys + 1 entries).
 * Device forms take device pointers (seeds, table, out_id included); sizes come back on the host.  PARITY UNPINNED vs VTK. */
int ivx_dev_mesh_region_labels(int64_t nverts, const int32_t *faces, int64_t ntris, int32_t *tri_labels, int32_t *vert_labels,
                               int64_t *nregions, int64_t *nused_verts /* may be NULL */, void *stream);
int ivx_dev_mesh_split(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, float *out_verts,
                       int64_t max_verts, int32_t *out_faces, int64_t max_tris, int64_t *table, int64_t max_parts,
                       int64_t *out_nverts, int64_t *nparts, void *stream);
int ivx_dev_mesh_parts_mass(const float *verts, const int32_t *faces, const int64_t *table, int64_t nparts, int64_t ntris,
                            int64_t small_max, double *out, void *stream);
int ivx_dev_mesh_select_seeded(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const int32_t *seeds,
                               int64_t nseeds, float *out_verts, int64_t max_verts, int32_t *out_faces, int64_t max_tris,
                               int64_t *out_nverts, int64_t *out_ntris, void *stream);
int ivx_dev_mesh_nearest_point(const float *verts, int64_t nverts, const double *xyz /* host */, int32_t *out_id, void *stream);
int ivx_dev_partition_u32(const uint32_t *keys, int64_t n, uint32_t nkeys, uint32_t *order, uint32_t *offsets, void *stream);
int ivx_mesh_region_labels(int64_t nverts, const int32_t *faces, int64_t ntris, int32_t *tri_labels, int32_t *vert_labels,
                           int64_t *nregions);
int ivx_mesh_split(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, float *out_verts, int32_t *out_faces,
                   int64_t *table, int64_t *out_nverts, int64_t *nparts);
int ivx_mesh_parts_mass(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const int64_t *table,
                        int64_t nparts, double *out);
int ivx_mesh_select_seeded(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const int64_t *seeds,
                           int64_t nseeds, float *out_verts, int32_t *out_faces, int64_t *out_nverts, int64_t *out_ntris);
int ivx_mesh_nearest_point(const float *verts, int64_t nverts, const double *xyz, int64_t *id);

/* ------------------------------------------------------------------------------------------------
 * the geodesic measure: shortest paths along the triangle edges of the indexed surface (csrc/k_meshgeo.hip)
 *   replaces GeodesicMeasure._draw_line        invesalius/data/measures.py:1202-1256
 *            (vtkDijkstraGraphGeodesicPath between consecutive picks, each snapped with vtkPointLocator.FindClosestPoint:
 *             ivx_*_mesh_nearest_point above; the summed edge length is the measure's value in mm)
 * Mesh graph.  The unique neighbours of every point in ascending id order, as a CSR in a caller-owned device buffer that is
 * built once per mesh and read by every measure on it.  Neighbours come from the triangle sides, both directions; a side
 * whose two ids are equal (a degenerate triangle) is no edge; a point no triangle uses has an empty list; the valence is
 * not bounded.  The buffer holds int64 header[32] = {magic, nverts, ntris, stored neighbours, byte offset of the offsets,
 * byte offset of the neighbours}, then uint32 offsets[nverts + 1], then the uint32 neighbour ids.
 *   ivx_mesh_graph_bytes       an upper bound on the buffer's size for such a mesh
 *   ivx_dev_mesh_graph_build   fills it (too small a buffer: IVX_ERANGE, "room for")
 * Weights.  w(u, v) = sqrt((dx dx + dy dy) + dz dz) in float64 from the float32 positions widened to double, the root
 * correctly rounded, nothing contracted; computed on the fly.  Coincident points joined by a side give zero-length edges,
 * and those are edges.
 * Distances.  dist[v] is the least fixed point of d[v] = min_u fl(d[u] + w(u, v)) with d[source] = 0: since fl(a + w) is
 * monotone in a and never below a, no order of relaxation changes a bit of it (pinned to scipy.sparse.csgraph.dijkstra
 * under array_equal).  Points the source does not reach get +inf and pred -1; the source gets 0 and pred -1.
 *   delta            only frontier points below a threshold relax; when none is left the threshold moves to (smallest
 *                    waiting distance) + delta.  +inf: plain frontier relaxation; tiny: Dijkstra's order; <= 0: the default,
 *                    4 x the mesh's mean edge length (summed on the device in a fixed order, so the same from run to run).
 *   rounds_per_look  rounds queued between two looks of the host at the device's "anything left" word (<= 0: the default, 16).
 *                    Both defaults are the pair with the lowest median in the measured sweep of DESIGN 7j.
 *   stop_at >= 0     a point whose distance is not below the current dist[stop_at] does not relax.  dist[stop_at] and every
 *                    entry <= dist[stop_at] are exact then; ENTRIES ABOVE IT ARE UPPER BOUNDS OR +inf.  < 0: the whole field.
 *   pred             recorded when a point's distance is lowered: among the neighbours whose offer won that round, the
 *                    smallest id (ties between equal offers are therefore deterministic, and the predecessor graph stays
 *                    acyclic across zero-length edges -- a rule applied after the fact would cycle there).  pred is the same
 *                    from run to run for the same mesh, delta and rounds_per_look; BETWEEN SCHEDULES IT MAY DIFFER where two
 *                    paths are equally short.  May be NULL.
 *   stats            host int64[4], may be NULL: rounds, point relaxations, threshold advances, host looks.
 * Rounds stop at 4 nverts + 64 and the back-trace at nverts steps: a wrong frontier is IVX_EHIP, never a hang.
 * Path.  For every consecutive pair of ids: the distances with stop_at = the pair's end, then pred walked back from the end
 * on the device; `path` (device int32[max_path]) takes the ids from START to END, segment after segment, seg_points[i] how
 * many and seg_length[i] = dist[end].  At convergence fl(dist[pred[v]] + w) == dist[v], so seg_length equals the float64 sum
 * of the path's edge lengths accumulated from the start, bit for bit.  start == end: one id, length 0.0; an end that cannot
 * be reached: no ids, length +inf.  ids, seg_points, seg_length and stats are host arrays.
 * Errors, before any launch: an id (source, stop_at, ids[]) outside [0, nverts) IVX_EDOM; nids < 2 IVX_EINVAL; a mesh too
 * large for 32-bit ids IVX_EINVAL; too small a max_path IVX_ERANGE ("room for", known once the segment has been traced).
 * Host forms take host pointers and the faces: they upload, build the graph, run and download (face ids are checked: IVX_EDOM).
 * PARITY UNPINNED vs VTK; distances pinned to scipy: the reference sums the same edges in its filter's output order into one
 * running double over all segments, which can differ from the sum of seg_length in the last bits; VTK is not installed here. */
int ivx_mesh_graph_bytes(int64_t nverts, int64_t ntris, size_t *bytes);
int ivx_dev_mesh_graph_build(const int32_t *faces, int64_t nverts, int64_t ntris, void *graph, size_t graph_bytes, void *stream);
int ivx_dev_mesh_geodesic_distances(const float *verts, int64_t nverts, const void *graph, int64_t source, int64_t stop_at,
                                    double delta, int rounds_per_look, double *dist, int32_t *pred, int64_t *stats, void *stream);
int ivx_dev_mesh_geodesic_path(const float *verts, int64_t nverts, const void *graph, const int32_t *ids, int64_t nids,
                               int32_t *path, int64_t max_path, int64_t *seg_points, double *seg_length, int64_t *stats,
                               void *stream);
int ivx_mesh_geodesic_distances(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, int64_t source,
                                int64_t stop_at, double delta, int rounds_per_look, double *dist, int32_t *pred, int64_t *stats);
int ivx_mesh_geodesic_path(const float *verts, int64_t nverts, const int32_t *faces, int64_t ntris, const int32_t *ids,
                           int64_t nids, int32_t *path, int64_t max_path, int64_t *seg_points, double *seg_length, int64_t *stats);

/* ------------------------------------------------------------------------------------------------
 * context-aware smoothing of the indexed surface
 *   replaces context_aware_smoothing           invesalius_rs/src/mesh_py.rs:7-330 -> mesh.rs:27-86
 *            (python: invesalius_rs.Mesh.ca_smoothing / ca_smoothing, invesalius_rs/__init__.py:220-275;
 *             caller: join_process_surface, invesalius/data/surface_process.py:313-317)
 * verts: (nverts,3) IVX_F32 or IVX_F64, smoothed IN PLACE; faces: (ntris,3) int32 (the reference's (M,4) rows minus
 * their leading count column, which must be 3); normals: (ntris,3) float64 cell normals; t / tmax / bmin / n_iters as in
 * the reference ("angle", "max distance", "min weight", "steps").  Optional outputs (NULL to skip): the staircase
 * flags (nverts bytes) and the per-vertex weights (nverts doubles).  Results are bit-identical to a statement-by-
 * statement restatement of mesh.rs (oracle/ivx_oracle_mesh.c), its quirks included.
 *   ivx_*_mesh_propagate_weights  propagate_weights (mesh.rs:204-288) alone, from explicit seed flags
 *   ivx_*_mesh_face_normals       unit cell normals of the triangles (what vtkPolyDataNormals hands the reference)
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_context_aware_smoothing(void *verts, int vdtype, int64_t nverts, const int32_t *faces, int64_t ntris,
                                    const double *normals, double t, double tmax, double bmin, int n_iters,
                                    uint8_t *staircase_out, double *weights_out, void *stream);
int ivx_dev_mesh_propagate_weights(const void *verts, int vdtype, int64_t nverts, const int32_t *faces, int64_t ntris,
                                   const uint8_t *seed_flags, double tmax, double bmin, double *weights, void *stream);
int ivx_dev_mesh_face_normals(const void *verts, int vdtype, const int32_t *faces, int64_t ntris, double *normals,
                              void *stream);
/* host forms; normals == NULL -> computed from the geometry */
int ivx_context_aware_smoothing(void *verts, int vdtype, int64_t nverts, const int32_t *faces, int64_t ntris,
                                const double *normals, double t, double tmax, double bmin, int n_iters,
                                uint8_t *staircase_out, double *weights_out);
int ivx_mesh_propagate_weights(const void *verts, int vdtype, int64_t nverts, const int32_t *faces, int64_t ntris,
                               const uint8_t *seed_flags, double tmax, double bmin, double *weights);
int ivx_mesh_face_normals(const void *verts, int vdtype, int64_t nverts, const int32_t *faces, int64_t ntris,
                          double *normals);

/* ------------------------------------------------------------------------------------------------
 * 3-D mask editing (callers: invesalius/data/mask3d_editor_state.py:176,221,259)
 *   ivx_*_mask_cut       replaces mask_cut        invesalius_rs/src/mask_cut_py.rs:9-69 -> mask_cut.rs:7-61
 *                        out (dz,dy,dx) uint8 edited in place; mask2d (mh,mw) bytes (numpy bool); m, mv 4x4 row-major
 *                        float64 (world->screen, world->camera); edit_mode 0 = include, 1 = exclude
 *   ivx_*_brush_mask     replaces brush_mask_rs   invesalius_rs/src/brush_mask_py.rs:8-28 -> brush_mask.rs:5-71
 *                        orig may be NULL (edit_mode 0 then paints 255)
 *   ivx_*_polygon2mask   replaces polygon2mask_rs invesalius_rs/src/polygon_mask_py.rs:7-27 -> polygon_mask.rs:4-79
 *                        out (w,h) bytes; points (npts,2) float64
 *   ivx_*_count_regions  replaces count_regions   invesalius_rs/src/count_regions_py.rs:9-26 -> count_regions.rs:5-18
 *                        labels IVX_I16 / IVX_I32 / IVX_I64; IVX_ERANGE where the reference panics (label outside
 *                        [0, number_regions])
 * Host forms take numpy-style byte strides.
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_mask_cut(uint8_t *out, int64_t dz, int64_t dy, int64_t dx, double sx, double sy, double sz, double max_depth,
                     const uint8_t *mask2d, int64_t mh, int64_t mw, const double *m, const double *mv, int edit_mode,
                     void *stream);
int ivx_dev_brush_mask(uint8_t *out, const uint8_t *orig, int64_t dz, int64_t dy, int64_t dx, const double spacing[3],
                       const double center[3], double radius, int edit_mode, void *stream);
/* points_dev: device copy read by the kernel; points_host: the same points on the host (bounding box) */
int ivx_dev_polygon2mask(int64_t w, int64_t h, const double *points_dev, const double *points_host, int64_t npts,
                         uint8_t *out, void *stream);
/* counts: device scratch of number_regions + 1 words; status: device int, non-zero after the call = label out of range */
int ivx_dev_count_regions(int ldtype, const void *labels, int64_t n, int64_t number_regions, uint32_t *counts,
                          uint32_t *out, int *status, void *stream);
int ivx_mask_cut(uint8_t *out, const int64_t shape[3], const int64_t out_strides[3], double sx, double sy, double sz,
                 double max_depth, const uint8_t *mask2d, int64_t mh, int64_t mw, const int64_t mask_strides[2],
                 const double *m, const double *mv, int edit_mode);
int ivx_brush_mask(uint8_t *out, const int64_t shape[3], const int64_t out_strides[3], const uint8_t *orig,
                   const int64_t orig_strides[3], const double spacing[3], const double center[3], double radius,
                   int edit_mode);
int ivx_polygon2mask(int64_t w, int64_t h, const double *points, int64_t npts, uint8_t *out);
int ivx_count_regions(int ldtype, const void *labels, const int64_t shape[3], const int64_t label_strides[3],
                      int64_t number_regions, uint32_t *out);

/* ------------------------------------------------------------------------------------------------
 * Slice editing tools (csrc/k_slice_edit.hip, csrc/slice_edit_math.h)
 *   ivx_*_mask_brush_stroke  the array work the three brushes share: Slice.edit_mask_pixel invesalius/data/slice_.py:656-744
 *                            (operations 0 .. 5 = BRUSH_DRAW, ERASE, THRESH, THRESH_ERASE, THRESH_ADD_ONLY, THRESH_ERASE_ONLY,
 *                            invesalius/constants.py:341-346), WaterShedInteractorStyle.edit_mask_pixel styles.py:2000-2069
 *                            and BaseImageEditionInteractorStyle.edit_mask_pixel styles.py:392-461 (operation 6 = IVX_BRUSH_FILL:
 *                            write `fill_value`).  `dabs` holds one (xi, yi) pair per dab: the first column and row of the
 *                            footprint's UNCLIPPED window on the slice, ``int(px - w + (w / 2 + 1))`` (slice_.py:690-695;
 *                            slice_edit_math.h computes it); a footprint pixel that falls outside the h x w slice is skipped
 *                            by the kernel, which is what the reference's four clips (:697-709) leave, and a window that
 *                            misses the slice writes nothing.  One operation per device call; the dabs of a call may overlap
 *                            (the result is that of the dabs applied one after another).  thresh_min / thresh_max: the
 *                            edition threshold range as integers (ceil / floor of the python numbers).
 *       device form: a 2-D view of the slice -- `mask` points at pixel (0, 0), strides are signed bytes (a sagittal view has
 *                    an element stride of one row pitch and a row stride of one plane) -- the matching int16 image view, or
 *                    NULL for the operations that do not read it (DRAW, ERASE, FILL); footprint fh x fw bytes (non-zero =
 *                    painted) and dabs in device memory.
 *       host form:   the padded (dz+1, dy+1, dx+1) mask matrix with its byte strides (or, padded = 0, a matrix of the image's
 *                    own shape: the watershed markers), the image matrix (image_shape is ITS shape; image may be NULL when no
 *                    run reads it), orientation 0 AXIAL / 1 CORONAL / 2 SAGITAL and slice n.  The dabs come in `nruns` runs of
 *                    one operation each (run_ops[r], run_lens[r] dabs), launched in order.  Only the slice is staged (from the
 *                    mirror when the matrix is registered, ivx_host_register) and written back to host and mirror;
 *                    set_flag: the slice's flag cell becomes 2 in both, the flag part of Slice.apply_slice_buffer_to_mask
 *                    (slice_.py:1925-1967); previous: NULL, or h * w bytes that receive the slice as it was before (p_mask).
 *   ivx_*_mask_crop          CropMaskInteractorStyle.CropMask styles.py:2654-2694: every byte of the (dz, dy, dx) block
 *                            outside box = {z0, z1, y0, y1, x0, x1} (half-open) becomes 1.  The host form takes the whole
 *                            padded matrix (flag planes included, as the reference's ``matrix[:] = 1``).
 * ---------------------------------------------------------------------------------------------- */
#define IVX_BRUSH_FILL 6
int ivx_dev_mask_brush_stroke(uint8_t *mask, int64_t mask_row_stride, int64_t mask_elem_stride, const int16_t *image,
                              int64_t image_row_stride, int64_t image_elem_stride, int64_t h, int64_t w, const uint8_t *footprint,
                              int64_t fh, int64_t fw, const int32_t *dabs, int64_t ndabs, int operation, int thresh_min,
                              int thresh_max, int fill_value, void *stream);
int ivx_mask_brush_stroke(uint8_t *mask, const int64_t image_shape[3], const int64_t mask_strides[3], const int16_t *image,
                          const int64_t image_strides[3], int orientation, int64_t n, const uint8_t *footprint, int64_t fh,
                          int64_t fw, const int32_t *dabs, const int32_t *run_ops, const int64_t *run_lens, int64_t nruns,
                          int thresh_min, int thresh_max, int fill_value, int padded, int set_flag, uint8_t *previous);
/* slice_edit_math.h for host callers (pure host code, no device): a flat integer position as (px, py); the (xi, yi) windows of
 * `ndabs` (px, py) positions; the four clips of one window, out = {x at, x skip, x count, y at, y skip, y count}; and what the
 * kernel's bounds test leaves of one dab in a view with these strides, out = {pixels, lowest, highest byte offset (-1: none)} */
int ivx_slice_flat_position(int64_t position, int64_t slice_width, double out_xy[2]);
int ivx_slice_dab_windows(const double *positions_xy, int64_t ndabs, int64_t fh, int64_t fw, int32_t *dabs);
int ivx_slice_dab_clip(int64_t xi, int64_t yi, int64_t fh, int64_t fw, int64_t h, int64_t w, int64_t out[6]);
int ivx_slice_dab_extent(int64_t xi, int64_t yi, int64_t fh, int64_t fw, int64_t h, int64_t w, int64_t row_stride,
                         int64_t elem_stride, int64_t out[3]);
int ivx_dev_mask_crop(uint8_t *mask, int64_t dz, int64_t dy, int64_t dx, const int64_t box[6], void *stream);
int ivx_mask_crop(uint8_t *mask, const int64_t shape[3], const int64_t mask_strides[3], const int64_t box[6]);

/* ------------------------------------------------------------------------------------------------
 * image geometry tools: the three operations of the reference that rewrite the whole image
 *   flip          Slice.OnFlipVolume (invesalius/data/slice_.py:2103-2149): m[:] = m[::-1] on axis 0 / 1 / 2 of (z, y, x)
 *   swap axes     Slice.OnSwapVolumeAxes (:2151-2251): np.array(m.swapaxes(a, b)), a new block of the new shape
 *   gantry tilt   imagedata_utils.FixGantryTilt (imagedata_utils.py:143-154): slice n becomes
 *                 scipy.ndimage.shift(slice, (shifts[n], 0), order 3, mode "constant", cval = the matrix's minimum as it
 *                 stands before slice n), int16, bit for bit (csrc/imagegeo_math.h has the arithmetic)
 * `itemsize` 1 / 2 / 4 / 8: flip and swap move elements, whatever they mean.  The _dev_ forms work on dense device blocks
 * and enqueue on `stream`; flip and tilt work in place, swap writes `dst` (same number of elements; `src` and `dst` must not
 * overlap).  The host forms take host views (signed byte strides) through the copy helpers, so a registered array comes from
 * its mirror and the result goes to the host and the mirror.
 * Tilt: `shifts` is a HOST array of dz doubles, the first component of the shift the reference hands scipy for each slice.
 * The device form needs `scratch`, 8-byte aligned: ivx_image_tilt_scratch_bytes reports the size it likes (a head of
 * 20 bytes per slice rounded up to 256, then float64 coefficients for as many slices as fit 512 MiB); anything from the
 * head plus ONE slice of coefficients (dy * dx * 8 bytes) is accepted -- more only lets a launch take more slices, the
 * result does not depend on it.  It waits for `stream` once in the middle (the per-slice minima come to the host, where
 * the chain of fill values is resolved) and returns with the fill pass queued.  `cvals_out` (host, dz ints, or NULL)
 * receives the fill value of every slice.
 * ivx_host_zero: memset(p, 0, nbytes) on the host and, where [p, p + nbytes) lies in a registered range, the same in its
 * mirror -- no byte crosses the link (what the tools above do with every mask).  ivx_host_register_zero registers a range
 * like ivx_host_register but uploads nothing: the mirror starts as zeros, and so must the host range (or the caller lets a
 * host form of this header write all of it next).
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_image_flip(void *vol, int64_t dz, int64_t dy, int64_t dx, size_t itemsize, int axis, void *stream);
int ivx_image_flip(void *vol, const int64_t shape[3], const int64_t strides[3], size_t itemsize, int axis);
int ivx_dev_image_swap_axes(const void *src, int64_t dz, int64_t dy, int64_t dx, size_t itemsize, int axis_a, int axis_b, void *dst,
                            void *stream);
int ivx_image_swap_axes(const void *src, const int64_t shape[3], const int64_t strides[3], size_t itemsize, int axis_a, int axis_b,
                        void *dst, const int64_t dst_strides[3]);
int ivx_image_tilt_scratch_bytes(int64_t dz, int64_t dy, int64_t dx, size_t *nbytes);
int ivx_dev_image_fix_gantry_tilt(int16_t *vol, int64_t dz, int64_t dy, int64_t dx, const double *shifts, void *scratch,
                                  size_t scratch_bytes, int *cvals_out, void *stream);
int ivx_image_fix_gantry_tilt(int16_t *vol, const int64_t shape[3], const int64_t strides[3], const double *shifts, int *cvals_out);
int ivx_host_zero(void *p, size_t nbytes);
int ivx_host_register_zero(const void *base, size_t nbytes, uint64_t *handle);

/* ------------------------------------------------------------------------------------------------
 * mask edit history (csrc/k_maskhist.hip, csrc/mask_history_math.h): volume snapshots of a mask's bytes for
 * EditionHistory (invesalius/data/mask.py:40-203), kept in HBM in the `blocks64` format.  A dense stream of n bytes is cut
 * into B = ceil(n / 64) blocks of 64 bytes and W = ceil(B / 64) words of 64 blocks.
 *   header  value[B] u8 (the block's first byte; padded with zeros to a multiple of 8 bytes), literal[W] u64 (bit b of
 *           word w set <=> block 64 w + b holds a byte, at an offset < n, that differs from its first byte), base[W] u32
 *           (literal blocks before word w).  Its size depends on n alone: ivx_mask_snapshot_header_bytes.
 *   pool    the L literal blocks in stream order, 64 bytes each; bytes of the last block past n are stored as 0.
 * Device forms (blocks in device memory, enqueued on `stream`; header 8-byte and pool 16-byte aligned, src / dst any):
 *   scan     one pass over src: writes the header and returns L on the host -- it waits for `stream` once, because the
 *            pool is sized from L.  Reads no byte at or past src + n.
 *   pack     copies the literal blocks into `pool` (room for literal_blocks * 64 bytes).
 *   restore  decodes the snapshot, compares with what dst holds and stores only where a byte differs; never a byte at or
 *            past dst + n.  plane_flags (ceil(n / plane_bytes) bytes, zeroed by the caller; may be NULL): byte p becomes 1
 *            for every plane p = offset / plane_bytes that holds a differing byte.
 * Host forms take the C-contiguous host bytes of the matrix.  A matrix inside a registered range (ivx_host_register) is
 * encoded straight from its mirror; any other one is staged once.  ivx_mask_snapshot returns header and pool as device
 * blocks the caller frees with ivx_free.  ivx_mask_snapshot_restore on a registered matrix restores into the mirror and
 * copies each run of consecutive changed planes mirror -> host (counted by ivx_transfer_stats; the flags themselves are a
 * small argument and are not), so both hold the same bytes afterwards; on any other matrix all n bytes are decoded and
 * downloaded.  *planes_written (may be NULL) = planes copied to the host.
 * ---------------------------------------------------------------------------------------------- */
int ivx_mask_snapshot_header_bytes(int64_t n, size_t *nbytes);
int ivx_dev_mask_snapshot_scan(const uint8_t *src, int64_t n, void *header, int64_t *literal_blocks, void *stream);
int ivx_dev_mask_snapshot_pack(const uint8_t *src, int64_t n, const void *header, void *pool, int64_t literal_blocks, void *stream);
int ivx_dev_mask_snapshot_restore(uint8_t *dst, int64_t n, const void *header, const void *pool, int64_t literal_blocks,
                                  int64_t plane_bytes, uint8_t *plane_flags, void *stream);
int ivx_mask_snapshot(const uint8_t *matrix, size_t nbytes, void **header, void **pool, int64_t *literal_blocks);
int ivx_mask_snapshot_restore(uint8_t *matrix, size_t nbytes, const void *header, const void *pool, int64_t literal_blocks,
                              size_t plane_bytes, int64_t *planes_written);

/* ------------------------------------------------------------------------------------------------
 * whole-mask numpy expressions of invesalius/data/slice_.py
 *   ivx_*_mask_boolean        Slice.do_boolean_op slice_.py:1906-1916: out = 255 where op(m1 > 2, m2 > 2) else 0;
 *                             op = 1 union, 2 diff (m1 and not m2), 3 intersection, 4 xor (constants.py:818-821)
 *   ivx_*_masked_density_i16  Slice.calc_image_density slice_.py:2284-2297: count / sum / sum of squares (exact
 *                             integers) / min / max of the int16 image where mask > 127; mean and std are formed
 *                             from them in float64 by the caller
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_mask_boolean(int op, const uint8_t *m1, const uint8_t *m2, uint8_t *out, int64_t n, void *stream);
/* acc5: 32 bytes on the device: int64 count, sum, sum of squares, then int32 min, max */
int ivx_dev_masked_density_i16(const int16_t *img, const uint8_t *mask, int64_t n, void *acc5, void *stream);
int ivx_mask_boolean(int op, const uint8_t *m1, const int64_t st1[3], const uint8_t *m2, const int64_t st2[3], uint8_t *out,
                     const int64_t sto[3], const int64_t shape[3]);
int ivx_masked_density_i16(const int16_t *img, const int64_t img_strides[3], const uint8_t *mask,
                           const int64_t mask_strides[3], const int64_t shape[3], double *out5);

/* ------------------------------------------------------------------------------------------------
 * convolve_non_zero and the mask-area measurement built on it
 *   ivx_*_convolve_non_zero  replaces convolve_non_zero  invesalius_rs/src/transforms_py.rs:51-93
 *                            (float64 volume and kernel; correlation, outside = cval (an int16), zero where the
 *                            volume is zero; every output value bit-identical to the reference's (k, j, i) sum)
 *   ivx_*_mask_area          replaces Slice.calc_image_area  invesalius/data/slice_.py:2296-2322  (mask > 127, the
 *                            7-point exposed-face kernel of the spacing, cval = 1, summed) without materialising
 *                            the float64 volume; spacing = (sx, sy, sz)
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_convolve_non_zero(const double *volume, int64_t sz, int64_t sy, int64_t sx, const double *kernel, int64_t skz,
                              int64_t sky, int64_t skx, int cval, double *out, void *stream);
int ivx_mask_area_scratch_bytes(int64_t sz, int64_t sy, int64_t sx, size_t *nbytes);
/* kernel27_dev: the 27 doubles of the kernel on the device; area_dev: one double on the device */
int ivx_dev_mask_area_u8(const uint8_t *mask, int64_t sz, int64_t sy, int64_t sx, const double *kernel27_dev,
                         double *scratch, double *area_dev, void *stream);
int ivx_convolve_non_zero(const double *volume, const int64_t shape[3], const int64_t vol_strides[3], const double *kernel,
                          const int64_t kshape[3], int cval, double *out);
int ivx_mask_area(const uint8_t *mask, const int64_t shape[3], const int64_t mask_strides[3], const double spacing_xyz[3],
                  double *area);

/* ------------------------------------------------------------------------------------------------
 * seeded region growing
 *   replaces generic_floodfill_threshold          invesalius_rs/src/floodfill.rs:96-166
 *            generic_floodfill_threshold_inplace  invesalius_rs/src/floodfill.rs:168-237
 *   (bindings floodfill_py.rs:137-231, wrappers invesalius_rs/__init__.py:21-54)
 * Device form works on a bit-packed candidate / reached pair (1 bit per voxel, 64 voxels of an
 * x-row per uint64 word, rows padded to a whole word): see DESIGN.md "region growing".
 * ---------------------------------------------------------------------------------------------- */
typedef struct ivx_flood_plan {
    int64_t dz, dy, dx;
    int64_t wx;            /* uint64 words per x-row = ceil(dx/64) */
    uint32_t strct_bits;   /* bit (kk*9+jj*3+ii) set <=> strct[kk][jj][ii] != 0 (3x3x3, centre ignored) */
} ivx_flood_plan;
/* bytes of ONE bit volume (candidate or reached) for this plan */
int ivx_flood_bits_bytes(const ivx_flood_plan *p, size_t *nbytes);
/* scratch for the tile work-list */
int ivx_flood_scratch_bytes(const ivx_flood_plan *p, size_t *nbytes);
/* strct (dims 1..3 each, centre offset dim/2 as floodfill.rs:108-110) -> plan.strct_bits */
int ivx_flood_strct_bits(const uint8_t *strct, const int64_t sshape[3], uint32_t *bits);
/* zero `reached` and the tile work-list in `scratch` */
int ivx_dev_flood_clear(const ivx_flood_plan *p, uint64_t *reached, void *scratch, void *stream);
/* cand[v] = (t0 <= data[v] <= t1) && not blocked(v); barrier_mode 0: nothing blocks, 1: barrier[v] == (uint8)fill
 * blocks (out-of-place form, floodfill.rs:154), 2: data[v] == fill blocks (in-place form, floodfill.rs:225) */
int ivx_dev_flood_candidates(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                             const uint8_t *barrier, int barrier_mode, double fill, uint64_t *cand, void *stream);
/* The same plane for int16 data whose (min, max) records are valid (ivx_dev_image_ranges_i16; dx % 64 == 0 and 16-byte
 * aligned buffers, IVX_EINVAL otherwise): a word wholly outside [t0, t1] is written as 0 without a load, a word wholly
 * inside skips the image (and with barrier_mode 0 the barrier too).  barrier_mode 0 or 1.  The records are trusted. */
int ivx_dev_flood_candidates_ranges(const ivx_flood_plan *p, const int16_t *data, double t0, double t1,
                                    const uint8_t *barrier, int barrier_mode, double fill, const uint32_t *ranges,
                                    uint64_t *cand, void *stream);
/* reached := seeds (x,y,z triples on the HOST) that are in [t0,t1]; such seeds are also forced into cand
 * (a pre-filled seed still expands, floodfill.rs:121-128).  Out-of-bounds seed -> IVX_ERANGE. */
int ivx_dev_flood_seed(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                       const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand, uint64_t *reached,
                       void *scratch, void *stream);
/* grow `reached` inside `cand` to the fix-point; *rounds (host, may be NULL) = global rounds used */
int ivx_dev_flood_run(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, void *scratch,
                      int *rounds, void *stream);
/* ivx_dev_flood_clear + ivx_dev_flood_seed + ivx_dev_flood_run in one call: floodfill.rs:96-166 from `seeds` over `cand`
 * into `reached`, whose previous contents are discarded.  With <= 16 seeds and scipy's 6 / 18 / 26 structure the clearing
 * and the seeding ride on the coarse pass (no separate pass over the plane, two launches fewer); IVX_FLOOD_FUSED=0 runs the
 * three calls one after the other (same bits). */
int ivx_dev_flood_grow(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                       const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand, uint64_t *reached, void *scratch,
                       int *rounds, void *stream);
/* What the rounds of the last flood on `scratch` cost: out[0] = tile visits (the sum of the rounds' list lengths), out[1] =
 * the length of the first round's list.  Queue-ordered on `stream` (it waits for what the stream holds), one small read.
 * Only the rounds of tile visits count: when a long thin region went to the union-find engine after 48 rounds the figure
 * covers the rounds before that, and after a flood that ran no round at all (IVX_FLOOD_MODE=ccl) the two words are not
 * defined (that path does not touch the counters). */
int ivx_dev_flood_visits(const ivx_flood_plan *p, const void *scratch, uint32_t out[2], void *stream);
/* host only, for tests: the path ivx_dev_flood_grow takes for this plan and `nseeds` seeds, from the functions that size its
 * launches (no device call).  out[0] coarse pass on (0/1), out[1] block width in voxels along x (16 / 32 / 64), out[2] blocks
 * per tile along x, out[3] lanes of the coarse workgroup, out[4] rows of tiles per lane = ceil(rows / lanes) (out[1..4] are 0
 * with the coarse pass off), out[5] fused start taken for `nseeds` (0/1), out[6] the most workgroups a round is launched
 * with, out[7] tiles.  The IVX_FLOOD_* switches of the process count as they do for a flood. */
int ivx_flood_describe(const ivx_flood_plan *p, int64_t nseeds, int32_t out[8]);
/* Gate for background work (e.g. the next stage's mask-independent passes on a second, low-priority stream): the next
 * ivx_dev_flood_run on `scratch` stores `value` to the device word `word` from the first round that starts with fewer
 * than `below_tiles` tiles -- its throughput-bound head is over -- or when it returns, if no round did.
 * ivx_dev_gate_wait parks `stream` behind a one-wave kernel polling the word; it gives up after `timeout_us`. */
int ivx_dev_flood_arm_gate(const void *scratch, uint32_t *word, uint32_t value, uint32_t below_tiles);
/* drop an arm no flood has consumed (gate opened by hand / buffers about to be freed): the arm is keyed by the scratch
 * address, which a later allocation may reuse */
int ivx_dev_flood_disarm_gate(const void *scratch);
int ivx_dev_gate_wait(const uint32_t *word, uint32_t value, uint32_t timeout_us, void *stream);
int ivx_dev_gate_open(uint32_t *word, uint32_t value, void *stream); /* open it by hand (no flood came) */
/* mark every tile of the plan whose z-range touches [z0,z1) dirty (multi-GPU halo re-seeding) */
int ivx_dev_flood_mark_slab(const ivx_flood_plan *p, void *scratch, int64_t z0, int64_t z1, void *stream);
/* multi-GPU slab halo: reached[z] |= plane & cand[z] (plane = the Z-neighbour's boundary plane, dy*wx words);
 * *changed (host) = number of words that gained bits; the tiles touching z are re-marked dirty */
/* whole-plane dst |= src (op 0) / dst &= ~src (op 1) */
int ivx_dev_bits_combine(uint64_t *dst, const uint64_t *src, int64_t nwords, int op, void *stream);
int ivx_dev_flood_or_plane(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z,
                           const uint64_t *plane, void *scratch, int *changed, void *stream);
/* both halo planes of a slab in one call (either plane may be NULL): same update per plane, the tiles of the words that
 * gained bits are marked dirty on the device, ONE read-back: *changed (host) = words that gained bits in either plane */
int ivx_dev_flood_or_planes(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z_a,
                            const uint64_t *plane_a, int64_t z_b, const uint64_t *plane_b, void *scratch, int *changed,
                            void *stream);
/* the same with NO read-back: the count is left in the caller's DEVICE word, where ivx_comm_exchange_vote's all-reduce
 * reads it in the next round */
int ivx_dev_flood_or_planes_dev(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z_a,
                                const uint64_t *plane_a, int64_t z_b, const uint64_t *plane_b, void *scratch,
                                uint32_t *changed_dev, void *stream);
/* the same, the count ADDED to the caller's device word (ivx_dev_vote_read leaves it at zero: no fill per round) */
int ivx_dev_flood_or_planes_acc(const ivx_flood_plan *p, const uint64_t *cand, uint64_t *reached, int64_t z_a,
                                const uint64_t *plane_a, int64_t z_b, const uint64_t *plane_b, void *scratch,
                                uint32_t *changed_dev, void *stream);
/* out[v] = fill where reached (uint8 out), or data[v] = fill (in-place form, dtype of data) */
int ivx_dev_flood_apply(const ivx_flood_plan *p, const uint64_t *reached, int dtype, void *target,
                        double fill, void *stream);
/* mask[v] = v_sel where reached, for a uint8 mask whose bytes are KNOWN to be v_in where `inside_bits` (layout of `reached`)
 * has a bit and 0 elsewhere -- the mask and plane ivx_dev_threshold_i16_bits leaves, v_in = 255.  Same bytes afterwards as
 * ivx_dev_flood_apply(p, reached, IVX_U8, mask, v_sel, stream), reached bits outside the inside plane included, but the mask
 * is not read: a 16-voxel chunk with a reached bit is written from the two bit fields (v_sel where reached, else v_in where
 * inside, else 0), a chunk without one is left alone.  dx % 64 == 0 and a 16-byte aligned mask only (IVX_EINVAL). */
int ivx_dev_flood_apply_levels(const ivx_flood_plan *p, const uint64_t *reached, const uint64_t *inside_bits, uint8_t *mask,
                               int v_in, int v_sel, void *stream);
/* Every byte of a uint8 mask from its planes: v_sel where `reached` has a bit (NULL: nowhere), else v_in where `inside_bits`
 * has one, else 0.  Nothing of the mask is read and every 16-voxel chunk is written, so the mask may hold anything before:
 * after a plane-only threshold this is the threshold's mask (reached = NULL) or the mask after `mask[reached] = v_sel`.
 * dx % 64 == 0, a 16-byte aligned mask and 8-byte aligned planes only (IVX_EINVAL). */
int ivx_dev_mask_from_planes(const ivx_flood_plan *p, const uint64_t *inside_bits, const uint64_t *reached, uint8_t *mask,
                             int v_in, int v_sel, void *stream);
/* The write that follows a flood on its stream (ivx_dev_flood_grow_select): none, or one of the three single-kernel writes
 * above with the flood's `reached` plane -- ivx_dev_mask_from_planes(p, inside_bits, reached, mask, v_in, v_sel),
 * ivx_dev_flood_apply_levels(p, reached, inside_bits, mask, v_in, v_sel), ivx_dev_flood_apply(p, reached, IVX_U8, mask, v_sel).
 * Fields a kind does not use are ignored. */
enum { IVX_FLOOD_WRITE_NONE = 0, IVX_FLOOD_WRITE_MASK_FROM_PLANES = 1, IVX_FLOOD_WRITE_APPLY_LEVELS = 2, IVX_FLOOD_WRITE_APPLY_U8 = 3 };
typedef struct ivx_flood_write {
    int32_t kind, v_in, v_sel, reserved;
    const uint64_t *inside_bits;
    uint8_t *mask;
} ivx_flood_write;
/* ivx_dev_flood_grow, then `write` queued behind it from the same call: the host launches the write's kernel the moment it has
 * seen the flood end, so the GPU does not wait for the caller to learn of the end and come back with the write.  The write
 * lands behind whatever the flood queued last, on every path the flood can take (rounds, union-find escape, IVX_FLOOD_MODE=
 * ccl, the unfused start, a plan without tiles); same bits as the two calls one after the other.  The two writes from the
 * bit planes go one step further: while the rounds' lists run out the flood queues the write among its rounds, as a launch
 * that reads the next round's list length on the device and returns at once unless it is zero, so the write starts where
 * the first idle round would have, without the host in between (IVX_FLOOD_EARLY=0: only after the host has seen the end).  `look_ahead`: rounds the
 * host keeps queued beyond the newest one it has seen start, 0 .. 8; negative = the default, by the list length (see
 * ivx_flood_look_ahead); IVX_FLOOD_BATCH, if set, overrides either.  The rounds and *rounds do not depend on it.  If the flood fails nothing is
 * written; an error of the write is returned after a completed flood. */
int ivx_dev_flood_grow_select(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                              const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand, uint64_t *reached, void *scratch,
                              int *rounds, const ivx_flood_write *write, int look_ahead, void *stream);
/* ivx_dev_flood_grow_select for a flood that a surface call follows.  Marching cubes' count reads the inside plane only, and
 * nothing in the stream reads the bytes the write produces, so where `write` is one of the two writes from the bit planes
 * (and dx % 64 == 0 etc. as they require) every launch of it is one kernel that also counts the triangles of the piece `mc`
 * (one iso-value, ny == dy, nx == dx, nz <= dz; its inside plane is write->inside_bits from slice 0) into `mc_scratch`: the
 * count's dependent loads run under the write's stores.  The scan is queued behind the launch that went ahead and
 * *counted = 1: `mc_scratch` is then what ivx_dev_mc_count_bits_async(mc, write->inside_bits, mc_scratch, stream) leaves, and
 * ivx_dev_mc_list / _emit* / _total_early may follow.  Otherwise -- another write kind, a piece that does not fit, the
 * union-find escape, IVX_FLOOD_MODE=ccl -- the call is ivx_dev_flood_grow_select and *counted = 0.  Same mask bytes, same
 * counts as the separate calls. */
int ivx_dev_flood_grow_select_count(const ivx_flood_plan *p, int dtype, const void *data, double t0, double t1,
                                    const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand, uint64_t *reached, void *scratch,
                                    int *rounds, const ivx_flood_write *write, int look_ahead, const ivx_mc_params *mc,
                                    void *mc_scratch, int *counted, void *stream);
/* host only, for tests: the default look-ahead behind a round that starts with `n_list` tiles on its list */
int ivx_flood_look_ahead(int64_t n_list, int32_t *look_ahead);
/* both writes of a GUI region-grow in one pass: out[v] = fill and mask[v] = select where reached
 * (floodfill_threshold's out + `mask[out_mask.astype(bool)] = 254`, styles.py:3200-3214) */
int ivx_dev_flood_apply2(const ivx_flood_plan *p, const uint64_t *reached, uint8_t *out, int fill, uint8_t *mask,
                         int select, void *stream);
/* number of reached voxels */
int ivx_dev_flood_count(const ivx_flood_plan *p, const uint64_t *reached, int64_t *count, void *stream);
/* directed floods (floodfill_auto_threshold): six edge planes (+x, -x, +y, -y, +z, -z; bit = SOURCE voxel, layout of the
 * candidate plane, packed back to back) instead of a candidate plane.  ivx_dev_flood_edges_auto builds them for
 * floodfill_py.rs:32-35: from a voxel of value v the flood may step to a neighbour whose value lies in
 * [ceil(v(1-p)), floor(v(1+p))] (f32 products, `as i16`) and whose `out` byte is not `fill`. */
int ivx_flood_edges_bytes(const ivx_flood_plan *p, size_t *nbytes);
int ivx_dev_flood_edges_auto(const ivx_flood_plan *p, const int16_t *data, const uint8_t *out, float pfrac, int fill,
                             uint64_t *edges, void *stream);
/* seeds set unconditionally (floodfill.rs:21, floodfill_py.rs:30); cand may be NULL */
int ivx_dev_flood_seed_forced(const ivx_flood_plan *p, const int64_t *seeds_xyz, int64_t nseeds, uint64_t *cand,
                              uint64_t *reached, void *scratch, void *stream);
/* ivx_dev_flood_run over edge planes */
int ivx_dev_flood_run_edges(const ivx_flood_plan *p, const uint64_t *edges, uint64_t *reached, void *scratch, int *rounds,
                            void *stream);
/* Host forms.  floodfill (invesalius_rs/__init__.py:10 = floodfill_py.rs:88-135, floodfill.rs:5-49): 6-neighbour
 * component of data == v around (x, y, z), the seed filled whatever its value.  floodfill_auto_threshold
 * (invesalius_rs/__init__.py:57-65 = floodfill_py.rs:12-85): int16 data, seeds as (x, y, z) triples. */
int ivx_floodfill(int dtype, const void *data, const int64_t shape[3], const int64_t strides[3], int64_t x, int64_t y,
                  int64_t z, double v, int fill, uint8_t *out, const int64_t out_strides[3]);
int ivx_floodfill_auto_threshold(const int16_t *data, const int64_t shape[3], const int64_t strides[3],
                                 const int64_t *seeds_xyz, int64_t nseeds, float pfrac, int fill, uint8_t *out,
                                 const int64_t out_strides[3]);
/* jump_flooding (invesalius_rs/__init__.py:76-80 = floodfill_py.rs:262-275, floodfill.rs:298-507): Voronoi owners (int32,
 * 1-based site index, 0 = none) and float32 distance to the owning site, floor(log2(max dim)) double-buffered passes of
 * 26 taps; normalize != 0: sites move to their cells' integer centroids, distances are recomputed and divided by the
 * cell maximum.  sites = nsites rows of (z, y, x) int32 in HOST memory.  Device form: dense arrays, in place. */
int ivx_dev_jump_flooding(float *dist, int32_t *owners, const int64_t shape[3], const int32_t *sites_host, int64_t nsites,
                          int normalize, void *stream);
int ivx_jump_flooding(float *dist, const int64_t dist_strides[3], int32_t *owners, const int64_t owner_strides[3],
                      const int64_t shape[3], const int32_t *sites, int64_t nsites, int normalize);
int ivx_floodfill_threshold(int dtype, const void *data, const int64_t shape[3], const int64_t strides[3],
                            const int64_t *seeds_xyz, int64_t nseeds, double t0, double t1, int fill,
                            const uint8_t *strct, const int64_t sshape[3], uint8_t *out,
                            const int64_t out_strides[3]);
int ivx_floodfill_threshold_inplace(int dtype, void *data, const int64_t shape[3], const int64_t strides[3],
                                    const int64_t *seeds_xyz, int64_t nseeds, double t0, double t1,
                                    double fill, const uint8_t *strct, const int64_t sshape[3]);

/* ------------------------------------------------------------------------------------------------
 * fill small holes
 *   replaces fill_holes_automatically_internal invesalius_rs/src/floodfill.rs:51-94
 *   (labels come from scipy.ndimage.label on the host, invesalius/data/mask.py:529-531)
 * *modified = 1 when any label had 0 < size <= max_size (then voxels whose label size <= max_size -> 254,
 * label 0 included: faithful quirk).  A label > nlabels is IVX_ERANGE (the reference panics).
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_fill_holes(uint8_t *mask, const uint32_t *labels, int64_t n, uint32_t nlabels, uint32_t max_size,
                       uint32_t *sizes /* device, nlabels+1 */, int *status2 /* device: [0] modified, [1] error */,
                       void *stream);
int ivx_fill_holes_automatically(uint8_t *mask, const int64_t shape[3], const int64_t mask_strides[3],
                                 const uint32_t *labels, const int64_t label_strides[3], uint32_t nlabels,
                                 uint32_t max_size, int *modified);
/* Mask.fill_holes_auto (invesalius/data/mask.py:519-562) in one call: imask = ~(mask > 127), connected components of
 * imask under `strct` (what scipy.ndimage.label computes there), then the rule above -- without a label volume: the
 * result depends on the labels only through the component sizes.  strct: generate_binary_structure(3, 1|2|3) or a
 * (1,3,3) 4-/8-neighbour element for a (1,h,w) slice.  *modified = the bool the reference's call returns. */
int ivx_dev_fill_holes_auto(uint8_t *mask, int64_t dz, int64_t dy, int64_t dx, const uint8_t *strct, const int64_t sshape[3],
                            uint32_t max_size, int *modified, void *stream);
int ivx_fill_holes_auto(uint8_t *mask, const int64_t shape[3], const int64_t mask_strides[3], const uint8_t *strct,
                        const int64_t sshape[3], uint32_t max_size, int *modified);

/* ------------------------------------------------------------------------------------------------
 * watershed pre- and post-processing (the deterministic parts of do_watershed,
 * invesalius/data/watershed_process.py:19-60)
 *   ivx_dev_lut_u16        get_LUT_value / get_LUT_value_255 (imagedata_utils.py:540-564): np.piecewise on an
 *                          int16 array -> int16 (float64 expression truncated toward zero) -> .astype(uint16)
 *   ivx_dev_shift_min_u16  (image - image.min()).astype("uint16")   (watershed_process.py:47,55)
 *   ivx_dev_morph_gradient_u16  scipy.ndimage.morphological_gradient(size) == max - min filter, mode="reflect"
 *   ivx_dev_watershed_merge     merge rule of styles.py:2147-2152: tmp (labels 0/1/2) into mask
 *   ivx_watershed_prepare  host form: LUT or min-shift, then optional gradient, -> the uint16 cost image
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_lut_u16(const int16_t *img, int64_t n, double window, double level, int top255, uint16_t *out,
                    void *stream);
/* same LUT, int16 out: the image get_LUT_value_255 hands to floodfill_threshold in the "dynamic" / "confidence"
 * region-growing modes with use_ww_wl (invesalius/data/styles.py:3166-3171, 3222-3225) */
int ivx_dev_lut_i16(const int16_t *img, int64_t n, double window, double level, int top255, int16_t *out,
                    void *stream);
int ivx_dev_shift_min_u16(const int16_t *img, int64_t n, int imin, uint16_t *out, void *stream);
int ivx_dev_morph_gradient_u16(const uint16_t *in, int64_t dz, int64_t dy, int64_t dx, const int size[3],
                               uint16_t *out, void *stream);
int ivx_dev_watershed_merge(uint8_t *mask, const uint8_t *tmp, int64_t n, int overwrite, void *stream);
int ivx_watershed_prepare(const int16_t *img, const int64_t shape[3], const int64_t strides[3], int use_ww_wl,
                          double window, double level, const int gradient_size[3] /* NULL = none */, uint16_t *out);
int ivx_watershed_merge(uint8_t *mask, const int64_t shape[3], const int64_t mask_strides[3], const uint8_t *tmp,
                        const int64_t tmp_strides[3], int overwrite);

/* The IFT cost map level by level on bit planes: C[p] = min over paths from a marker of the largest arc |I(a) - I(b)|
 * (6 neighbours, scipy's linear-index neighbourhood) for every voxel of cost < the number of levels done; levels run until
 * `stop_frac` of the voxels are in or `max_levels` are done.  Other voxels keep the caller's value (0xFFFF).  Used by
 * ivx_dev_watershed_ift before its relaxation; needs dx % 64 == 0 and dy % 16 == 0 (IVX_EINVAL otherwise).
 * ivx_dev_sk_cost_levels: the same for the scikit-image branch's cost (largest image VALUE on the path, markers cost their own
 * value, lattice neighbours under `strct`): level c = what the markers of value <= c reach inside {image <= c}, on the
 * region-growing engine; stops after level 0 when that level holds < 5 % of the voxels (no plateau).  Needs dx % 64 == 0 and
 * 16-byte aligned image and markers (IVX_EINVAL otherwise). */
int ivx_dev_sk_cost_levels(const uint16_t *image, int mdtype, const void *markers, int64_t dz, int64_t dy, int64_t dx,
                           const uint8_t strct[27], uint16_t *C, int max_levels, double stop_frac, int *levels_done,
                           int64_t *reached, int64_t *rounds, void *stream);
int ivx_dev_ws_cost_levels(const uint16_t *cost_image, int mdtype, const void *markers, int64_t dz, int64_t dy, int64_t dx,
                           uint16_t *C, int max_levels, double stop_frac, int *levels_done, int64_t *reached,
                           int64_t *rounds, void *stream);
/* ------------------------------------------------------------------------------------------------
 * the marker flood of do_watershed's IFT branch
 *   replaces scipy.ndimage.watershed_ift(tmp_image, markers, bstruct) as called at
 *            invesalius/data/watershed_process.py:44-46,54-57 (3-D) and invesalius/data/styles.py:1958-1983 (one slice,
 *            shape (1, h, w) with the 3x3 structure in strct[9..17])
 * cost: uint16 (the LUT / min-shifted image above), markers int16 or int8 (>= 0; the reference passes 0 / 1 / 2),
 * strct: 3x3x3 uint8, symmetric (generate_binary_structure).  Labels come back in the markers' dtype (what scipy
 * returns) and/or as uint8 (what `mask[:] = tmp_mask` stores, watershed_process.py:58).  Arc weight |I(p)-I(q)|, path
 * cost = largest arc, LIFO inside a cost bucket, neighbours by linear index (row wrap-around like scipy): the
 * defect-free statement of NI_WatershedIFT, see k_wsift.hip.  cost_out (optional): the minimax cost map.
 * stats (optional, host): [0] relaxation rounds, [1] tile visits, [2] non-empty cost levels, [3] time stamps used,
 * [4] marker voxels, [5] entry voxels, [6] tiles, [7] LDS sweeps over all tile visits, [8..12] microseconds of: costs, zones, bucketing, level chain, labels.
 * The host form uploads / downloads dense C-order arrays.
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_watershed_ift(const uint16_t *cost, int mdtype, const void *markers, int64_t dz, int64_t dy, int64_t dx,
                          const uint8_t strct[27], void *out_labels /* markers' dtype, may be NULL */,
                          uint8_t *out_u8 /* may be NULL */, uint16_t *cost_out /* may be NULL */, int64_t stats[16],
                          void *stream);
int ivx_watershed_ift(int idtype /* IVX_U8 | IVX_U16 */, const void *input, const int64_t shape[3], int mdtype,
                      const void *markers, const uint8_t strct[27], void *output, uint16_t *cost_out, int64_t stats[16]);

/* ------------------------------------------------------------------------------------------------
 * the marker flood of do_watershed's scikit-image branch (algorithm == "Watershed", the GUI's default)
 *   replaces skimage.segmentation.watershed(tmp_image, markers, bstruct) as called at
 *            invesalius/data/watershed_process.py:36-39,49-52 (3-D) and invesalius/data/styles.py:1958,1975 (one slice,
 *            shape (1, h, w) with the 3x3 structure in strct[9..17]); no mask, no compactness, no watershed lines.
 * image: uint16 (the gradient of the LUT / min-shifted image; 65535 is refused), markers int16 or int8 (any non-zero
 * label, negative ones included), strct: 3x3x3 uint8, symmetric.  Labels come back in the markers' dtype, as int32
 * (scikit-image's output dtype) and / or as uint8 (what `mask[:] = tmp_mask` stores).  The serial rule -- pop the
 * smallest (image value, age), age = push counter, label at push time -- is evaluated without the heap: k_wssk.hip.
 * Marker voxels of equal image value are taken in raster order (scikit-image's heap takes them in an order that
 * depends on its array layout); stats[6] counts the tied neighbours in that order that carry different labels:
 * 0 = identical to scikit-image by construction.  cost_out (optional): the minimax map of image values.
 * stats (optional, host): [0] relaxation rounds, [1] tile visits, [2] non-empty levels, [3] generations, [4] marker
 * voxels, [5] generation-0 voxels, [6] tied markers of different labels, [7] frontier launches, [8..11] microseconds
 * of: costs, generation 0, level chain, labels, [12] basin relay launches, [13] generation steps, [14] launches that took a run of
 * small levels in one workgroup, [15] tile rounds of levels relaxed tile-wise.
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_watershed_sk(const uint16_t *image, int mdtype, const void *markers, int64_t dz, int64_t dy, int64_t dx,
                         const uint8_t strct[27], void *out_labels /* markers' dtype, may be NULL */,
                         int32_t *out_i32 /* may be NULL */, uint8_t *out_u8 /* may be NULL */,
                         uint16_t *cost_out /* may be NULL */, int64_t stats[16], void *stream);
int ivx_watershed_sk(int idtype /* IVX_U8 | IVX_U16 */, const void *input, const int64_t shape[3], int mdtype,
                     const void *markers, const uint8_t strct[27], int32_t *output, uint16_t *cost_out, int64_t stats[16]);

/* do_watershed (invesalius/data/watershed_process.py:19-60) in one host call: int16 image (dense or a strided view) and
 * markers (dense, int16 / int8) up once, uint8 labels (what `mask[:] = tmp_mask` stores) back once.  algorithm 0 =
 * "Watershed IFT" (LUT or min-shift -> ivx_dev_watershed_ift), 1 = "Watershed" (the same, then the morphological gradient of
 * gradient_size -> ivx_dev_watershed_sk).  stats as for the flood that ran. */
int ivx_do_watershed(const int16_t *img, const int64_t shape[3], const int64_t strides[3], int mdtype, const void *markers,
                     const uint8_t strct[27], int algorithm, const int gradient_size[3] /* NULL for algorithm 0 */,
                     int use_ww_wl, double window, double level, uint8_t *out_u8, int64_t stats[16]);
/* The same, as the Python hook calls it: `markers` in the caller's own integer dtype (IVX_U8 / I8 / I16 / U16 / I32 / I64, dense or a
 * sub-box view: byte strides) and cast on the device to `mdtype` (IVX_I16 | IVX_I8 -- watershed_process.py:39,45,52,57 do
 * `markers.astype("int16" | "int8")` on the host, two's-complement truncation like numpy); the uint8 labels are written through
 * `out_strides` straight into the caller's array -- the memmap of `tfile` (watershed_process.py:21,58) -- so the reference's
 * `mask[:] = tmp_mask` second pass over the volume does not exist. */
int ivx_do_watershed_into(const int16_t *img, const int64_t shape[3], const int64_t strides[3], int mk_src_dtype, const void *markers,
                          const int64_t mk_strides[3], int mdtype, const uint8_t strct[27], int algorithm,
                          const int gradient_size[3] /* NULL for algorithm 0 */, int use_ww_wl, double window, double level,
                          uint8_t *out_u8, const int64_t out_strides[3], int64_t stats[16]);

/* ------------------------------------------------------------------------------------------------
 * confidence-connected region growing support (do_rg_confidence, invesalius/data/styles.py:3220-3251):
 * exact integer count / sum / sum-of-squares of image[sel != 0]; dst[v] = 1 where src[v] == value.
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_masked_stats_i16(const int16_t *img, const uint8_t *sel, int64_t n, int64_t out3[3], void *stream);
int ivx_dev_or_equal_u8(uint8_t *dst, const uint8_t *src, int64_t n, int value, void *stream);
/* dst[v] = fill where src[v] == value  (mask[out_mask.astype(bool)] = 254, styles.py:3214,3249) */
int ivx_dev_flood_apply_where(uint8_t *dst, const uint8_t *src, int64_t n, int value, int fill, void *stream);

/* ------------------------------------------------------------------------------------------------
 * resample a slab through the 4x4 view matrix (re-oriented volumes, the step in front of the projections)
 *   replaces apply_view_matrix_transform  invesalius_rs/src/transforms_py.rs:12-49,95-147
 *            coord_transform               invesalius_rs/src/transforms.rs:9-55
 *            nearest / trilinear / tricubic / Lanczos-4 with single wrap-around  invesalius_rs/src/interpolation.rs
 * m is row-major; orientation 0/1/2 = AXIAL/CORONAL/SAGITAL adds n to z/y/x of the output index; minterpol
 * 0 nearest, 1 trilinear, 2 tricubic, else Lanczos; out has the volume's dtype.  A NumCast failure -> IVX_EDOM.
 * Lanczos on a volume with an axis of length 2: every voxel that falls inside is set to cval without a read and
 * raises IVX_EDOM on the same status word (the reference's tap -3 wraps to -1 and panics on the index).
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_apply_view_matrix_transform(int dtype, const void *vol, int64_t dz, int64_t dy, int64_t dx,
                                        const double spacing[3], const double m[16], int64_t n, int orientation,
                                        int minterpol, double cval, void *out, int64_t oz, int64_t oy, int64_t ox,
                                        int *status, void *stream);
int ivx_apply_view_matrix_transform(int dtype, const void *vol, const int64_t shape[3], const int64_t strides[3],
                                    const double spacing[3], const double m[16], int64_t n, int orientation,
                                    int minterpol, double cval, void *out, const int64_t oshape[3],
                                    const int64_t ostrides[3]);

/* ------------------------------------------------------------------------------------------------
 * quality-preset resample of the surface pipeline
 *   replaces imagedata_utils.resize_image_array (invesalius/data/imagedata_utils.py:121-130) =
 *            scipy.ndimage.zoom(image, factor, image.dtype, order=2), applied to image and mask by
 *            SurfaceManager.AddNewActor for the Low / Medium presets (invesalius/data/surface.py:1350-1353)
 * int16 or uint8 volumes, dense C order; oshape[a] = round(ishape[a] * factor) is the caller's (scipy's rule).
 * ---------------------------------------------------------------------------------------------- */
int ivx_zoom_scratch_bytes(const int64_t ishape[3], const int64_t oshape[3], size_t *nbytes);
int ivx_dev_zoom_order2(int dtype, const void *in, const int64_t ishape[3], void *out, const int64_t oshape[3],
                        void *scratch, void *stream);
int ivx_zoom_order2(int dtype, const void *in, const int64_t ishape[3], void *out, const int64_t oshape[3]);

/* ------------------------------------------------------------------------------------------------
 * image filters of the Image Filters dialog, int16 only (any other dtype -> IVX_EINVAL)
 *   replaces invesalius/data/filters.py:5-66 (gaussian_blur_filter, median_blur_filter, mean_blur_filter,
 *            sharpening_filter, despeckle_filter, border_detection_filter = scipy.ndimage gaussian_filter /
 *            median_filter / uniform_filter / sobel, mode "reflect") as dispatched by Slice.__apply_image_filter /
 *            _run_filter (invesalius/data/slice_.py:2330-2430), bit for bit with scipy 1.15.
 * kind: the reference's filter_type.  plane_axis -1 = the 3-D filter; 0/1/2 = "2D" with orientation Axial / Coronal /
 * Sagittal: every slice m[i], m[:, i] or m[:, :, i] filtered as a 2-D image (no pass along the slice axis, window extent
 * 1; sharpen's clip range and border detection's normalisation per slice).  A 2-D image is shape {1, h, w}, plane 0.
 * w, radius: the 2r+1 Gaussian weights exp(-0.5/sigma^2 x^2) / sum as numpy computes them (scipy's _gaussian_kernel1d,
 * r = int(4 sigma + 0.5)), read on the host; radius -1 = sigma <= 1e-15 (no pass).  Sharpen takes sigma 1's weights.
 * median size = max(3, min(int(2v + 1), 5)); mean size = int(2v + 1) (<= 1: identity); the ivx_dev_* forms take the
 * size, the host form the dialog's value.  Device buffers are dense C order; out must not alias in.
 * ---------------------------------------------------------------------------------------------- */
#define IVX_FILTER_GAUSSIAN 0
#define IVX_FILTER_MEDIAN 1
#define IVX_FILTER_MEAN 2
#define IVX_FILTER_SHARPEN 3
#define IVX_FILTER_DESPECKLE 4
#define IVX_FILTER_BORDER 5 /* Sobel magnitude of the Gaussian-smoothed image */
#define IVX_FILTER_MAX_RADIUS 255
int ivx_filter_scratch_bytes(int kind, const int64_t shape[3], int plane_axis, size_t *nbytes);
int ivx_dev_filter_gaussian_i16(const int16_t *in, const int64_t shape[3], int plane_axis, const double *w, int radius,
                                int16_t *out, void *scratch, void *stream);
int ivx_dev_filter_median_i16(const int16_t *in, const int64_t shape[3], int plane_axis, int size, int16_t *out,
                              void *stream);
int ivx_dev_filter_mean_i16(const int16_t *in, const int64_t shape[3], int plane_axis, int size, int16_t *out,
                            void *scratch, void *stream);
int ivx_dev_filter_sharpen_i16(const int16_t *in, const int64_t shape[3], int plane_axis, double value, const double *w,
                               int radius, int16_t *out, void *scratch, void *stream);
int ivx_dev_filter_border_i16(const int16_t *in, const int64_t shape[3], int plane_axis, int normalize, const double *w,
                              int radius, int16_t *out, void *scratch, void *stream);
int ivx_image_filter(int kind, double value, int plane_axis, int normalize, const double *w, int radius, int dtype,
                     const void *img, const int64_t shape[3], const int64_t strides[3], void *out,
                     const int64_t ostrides[3]);

/* ------------------------------------------------------------------------------------------------
 * deep-learning segmentation: the Unet3D of invesalius/segmentation/deep_learning/model.py:9-113 (brain MRI T1 and
 * trachea CT, BrainSegmentProcess / TracheaSegmentProcess, segment.py:505-541, 919-953), float32, eval mode.
 *   ivx_unet3d_load: network from a host float32 blob of FOLDED parameters (BatchNorm folded on the host in float64:
 *     w * g / sqrt(v + eps), (b - m) * g / sqrt(v + eps) + beta, rounded to float32 once), in this order:
 *       enc1, enc2, enc3, enc4, bottleneck: conv1 w (cout, cin, 5, 5, 5), conv1 b (cout), conv2 w, conv2 b;
 *       then for upconv4 / decoder4, upconv3 / decoder3, upconv2 / decoder2, upconv1 / decoder1:
 *         upconv w (cin, cout, 4, 4, 4) (torch's ConvTranspose3d layout), upconv b, conv1 w (cout, 2 cout, 5, 5, 5)
 *         (input channels: upsampled first, then the skip), conv1 b, conv2 w, conv2 b;
 *       final conv w (8), b (1).  ivx_unet3d_param_count gives the total.
 *   ivx_dev_unet3d_forward: the raw network on n patches of patch^3 (dense float32 in / out, patch a multiple of 16);
 *     the workspace holds some batch of patches and the call runs n in chunks of it.
 *   ivx_dev_unet3d_normalize: image_normalize(image, 0.0, 1.0, float32) (imagedata_utils.py:580-587) in numpy 2
 *     promotion, int16 wraps included; minmax2 = 2 device floats of scratch.
 *   ivx_dev_unet3d_segment: segment_torch's loop (segment.py:162-191) on the normalised volume: gen_patches' cuts,
 *     batches of `batch` patches, every voxel's covering cuts added in cut order onto prob (float32, read and written),
 *     then prob /= the cover count.  The result does not depend on `batch`.  progress (host, may be NULL) receives the
 *     fraction of cuts done after each batch.  Workspace: ivx_unet3d_workspace_bytes(net, patch, batch).
 *   ivx_dev_segment_threshold: apply_segment_threshold (segment.py:465-490): (prob >= threshold) * 255, float32
 *     comparison.  border = 1: mask is the (d+1, h+1, w+1) mask.matrix (strides in elements), written at [1:, 1:, 1:],
 *     and its lines [:, 0, 0], [0, :, 0], [0, 0, :] set to 2; border = 0: mask is the (d, h, w) interior alone.
 *   ivx_segment_unet3d: host form of _run_segmentation + segment_torch (int16 image of any strides, optional
 *     get_LUT_value(ww, wl), dense float32 prob in / out).
 * ---------------------------------------------------------------------------------------------- */
int ivx_unet3d_param_count(int64_t *nfloats);
int ivx_unet3d_load(const float *blob, int64_t nfloats, void **net);
int ivx_unet3d_free(void *net);
int ivx_unet3d_workspace_bytes(const void *net, int patch, int batch, size_t *nbytes);
int ivx_dev_unet3d_forward(const void *net, const float *in, int64_t n, int patch, float *out, void *workspace,
                           size_t ws_bytes, void *stream);
/* the forward once with a HIP event after each of its 27 launches (encoder: conv1, conv2, pool per level; bottleneck
 * conv1, conv2; decoder: upconv, conv1, conv2 per level; head); n patches must fit the workspace in one batch */
int ivx_unet3d_layer_times(const void *net, const float *in, int64_t n, int patch, float *out, void *workspace,
                           size_t ws_bytes, void *stream, float *ms /* 27 */);
/* diagnostic, for the tests: one layer of the network on its own, through the same weight packing and kernels the forward
 * uses.  Activations are channels-last device arrays (nb, S, S, S, C); w and bias are HOST arrays in torch layout.
 *   conv_layer: kind 0 = Conv3d(k 5, pad 2), w (cout, c0 + c1, 5, 5, 5), dst (nb, S, S, S, cout); kind 1 =
 *     ConvTranspose3d(k 4, s 2, p 1), w (c0 + c1, cout, 4, 4, 4), dst (nb, 2S, 2S, 2S, cout).  src1 / c1 are the second
 *     source of a torch.cat((src0, src1), 1) (NULL / 0 for none; then c0 must be a multiple of 4).  (mt, nt) forces
 *     the wave's tile shape, 16 mt voxels x 16 nt channels, to one of 1x1, 2x1, 4x1, 8x1, 2x2, 4x2, 4x4; (0, 0) takes the
 *     forward's own choice.  The shape used comes back in mt_used / nt_used.  IVX_EINVAL, before anything is launched,
 *     for any other pair and for one the forward never chooses for this cout (nt = 2 needs cout > 16, 4x4 cout > 48,
 *     8x1 cout <= 16).  Synchronises the stream.
 *   pool_layer: MaxPool3d(2), (nb, S, S, S, C) -> (nb, S/2, S/2, S/2, C), S even.
 *   head_layer: Conv3d(8 -> 1, k 1) + sigmoid, in (nvox, 8), w9 = 8 host weights then the bias, out (nvox). */
int ivx_dev_unet3d_conv_layer(int kind, const float *src0, int c0, const float *src1, int c1, const float *w,
                              const float *bias, int cout, int S, int nb, int relu, int mt, int nt, float *dst,
                              int *mt_used, int *nt_used, void *stream);
int ivx_dev_unet3d_pool_layer(const float *in, float *out, int S, int C, int nb, void *stream);
int ivx_dev_unet3d_head_layer(const float *in, const float *w9, int64_t nvox, float *out, void *stream);
int ivx_dev_unet3d_normalize(const int16_t *img, int64_t n, float *out, float *minmax2, void *stream);
int ivx_segment_cut_count(const int64_t shape[3], int patch, int overlap, int64_t *ncuts);
int ivx_dev_unet3d_segment(const void *net, const float *vol, const int64_t shape[3], int patch, int overlap, int batch,
                           float *prob, void *workspace, size_t ws_bytes, float *progress, void *stream);
int ivx_dev_segment_threshold(const float *prob, const int64_t shape[3], float threshold, uint8_t *mask,
                              const int64_t mstrides[3], int border, void *stream);
int ivx_segment_unet3d(const void *net, const int16_t *img, const int64_t shape[3], const int64_t strides[3],
                       int apply_wwwl, double window, double level, int patch, int overlap, int batch, float *prob,
                       float *progress);

/* ------------------------------------------------------------------------------------------------
 * volume rendering: the 3-D view's ray caster with the raycasting presets
 *   replaces invesalius/data/volume.py:575-707 (Volume.LoadVolume: vtkImageShiftScale, ApplyConvolution's
 *   vtkImageConvolve "Basic Smooth 5x5", vtkFixedPointVolumeRayCastMapper with a parallel camera) and
 *   CalculateHistogram (:723-735).  The contract (geometry, sampling, shading, compositing) is DESIGN.md section 7d; the
 *   tables come from invesalius3_amd/volume.py.  Device buffers are dense C order (z, y, x).
 * ivx_dev_volren_prepare   out = uint16(img + shift), then `nsmooth` passes of the 5x5 kernel (weights k / 60.0 in float64,
 *                          taps in row-major order, out-of-volume taps skipped, truncated toward zero) over every XY slice;
 *                          scratch: n uint16 when nsmooth >= 1 (else may be NULL); out must not alias img.
 * ivx_dev_volren_cells     per IVX_VOLREN_CELL^3 macro cell the min and max of the prepared field over the cell's voxels
 *                          plus one voxel on every side: cells[2 c] = min, cells[2 c + 1] = max, cell c = (cz, cy, cx) of a
 *                          grid of ceil(n / IVX_VOLREN_CELL) per axis.
 * ivx_dev_volren_render    one ray per pixel; table: n_table float4 (r, g, b, a' corrected for the sample distance),
 *                          alpha: n_table uncorrected a (MIP), prefix: n_table + 1 counts of entries with a' > 0; out:
 *                          height x width x 4 float32, or uint8 when out_u8; stats (optional, 4 uint64, accumulated):
 *                          samples classified, samples skipped, rays terminated early, rays that hit the box.
 * ivx_dev_volren_histogram counts[i] = voxels equal to lo + i for 0 <= i < nbins (uint64; zeroed here).
 * ivx_volume_render        host form: int16 image of any strides in, prepare + cells + render, the image out.
 * ---------------------------------------------------------------------------------------------- */
#define IVX_VOLREN_CELL 8
typedef struct ivx_volren_params {
    int32_t width, height; /* viewport in pixels; row 0 of out is the top */
    int32_t mip;           /* 0 composite (front to back), 1 maximum intensity */
    int32_t shade;         /* composite only: headlight shading with the four coefficients below */
    int32_t skip;          /* empty-space skipping over the macro cells (changes no bit of the result) */
    int32_t n_table;       /* entries of table / alpha (>= 2): scalar s reads entries floor(s), floor(s) + 1 */
    int32_t out_u8;        /* out is uint8 RGBA (floor(255 v + 0.5), clamped) instead of float32 RGBA */
    int32_t clip;          /* keep only n . (p - o) >= 0 of the clip plane below */
    double origin[3];      /* world position of pixel (0, 0)'s centre on the plane through the focal point */
    double du[3], dv[3];   /* world step per pixel column / per pixel row */
    double dir[3];         /* unit direction of the (parallel) rays */
    double spacing[3];     /* sx, sy, sz: voxel (z, y, x) sits at world (x sx, -y sy, z sz) */
    double dt;             /* sample distance along the ray (world units) */
    double ambient, diffuse, specular, specular_power;
    double background[3];  /* r, g, b in 0..1 */
    double clip_normal[3], clip_origin[3];
} ivx_volren_params;
int ivx_dev_volren_prepare(const int16_t *img, const int64_t shape[3], int shift, int nsmooth, uint16_t *out,
                           uint16_t *scratch, void *stream);
int ivx_dev_volren_cells(const uint16_t *vol, const int64_t shape[3], uint16_t *cells, void *stream);
int ivx_dev_volren_render(const uint16_t *vol, const uint16_t *cells, const int64_t shape[3], const float *table,
                          const float *alpha, const uint32_t *prefix, const ivx_volren_params *p, void *out,
                          uint64_t *stats, void *stream);
int ivx_dev_volren_histogram(const int16_t *img, int64_t n, int lo, int nbins, uint64_t *counts, void *stream);
int ivx_volume_render(const int16_t *img, const int64_t shape[3], const int64_t strides[3], int shift, int nsmooth,
                      const float *table, const float *alpha, const uint32_t *prefix, const ivx_volren_params *p,
                      void *out);

/* ------------------------------------------------------------------------------------------------
 * mask 3-D preview: ray casting of the uint8 mask, read in place
 *   replaces invesalius/data/volume_mask.py:36-119 (VolumeMask.create_volume: vtkFixedPointVolumeRayCastMapper, or
 *   vtkGPUVolumeRayCastMapper with the iso-surface blend mode at 127).  The contract is DESIGN.md section 7e; the tables
 *   and the camera come from invesalius3_amd/volume_mask.py.
 * The field: `mask` with `shape` (z, y, x) and byte `strides` of any sign.  With apron = 1 it is extended by one leading
 *   plane on every axis that holds the byte apron_value: logical index i reads array index i - 1, logical index 0 the
 *   constant (the dense resident mask then counts positions like the padded matrix with its flag planes).  Logical voxel
 *   (z, y, x) sits at world (x sx, -y sy, z sz) of ivx_volren_params, as for ivx_dev_volren_render: for the padded
 *   matrix the caller moves `origin` by (sx, -sy, sz), a translation that leaves the distances along the rays as they are.
 * ivx_dev_maskren_cells   per IVX_VOLREN_CELL^3 macro cell of the logical field the min and max byte over the cell's voxels
 *                         plus one voxel on every side: cells[2 c], cells[2 c + 1].  z1 < 0: every cell; else only the
 *                         cells that the logical slices [z0, z1) reach (a slab edit).
 * ivx_dev_maskren_render  iso = 0: the composite loop of ivx_dev_volren_render on bytes (p->mip and p->clip must be 0,
 *                         n_table >= 257; prefix counts as there, but READ MORE TIGHTLY: a cell is skipped when entries
 *                         [min, max] of its bytes are all transparent, not [min - 1, max + 1].  A sample s of a byte
 *                         field stays in [min, max] (every float32 lerp of the trilinear chain is monotone in its
 *                         rounding, so it cannot leave the range of its two integer ends), it reads entries floor(s) and
 *                         floor(s) + 1, and floor(s) + 1 > max only at s == max, where the fraction is 0 and that entry
 *                         weighs nothing.  So the table must be exact at integer s: a' of entry i is the opacity AT i).  iso = 1: the first crossing of 127 along the ray, shaded, with
 *                         alpha 1; `depth` (optional, height x width float32) receives the hit's distance from the pixel's
 *                         plane, +inf without a hit.  stats as for ivx_dev_volren_render (early = rays with a hit).
 * ivx_mask_preview        host form: a matrix of any strides in (no apron), cells + render, the image (and depth) out.
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_maskren_cells(const uint8_t *mask, const int64_t shape[3], const int64_t strides[3], int apron,
                          int apron_value, int64_t z0, int64_t z1, uint8_t *cells, void *stream);
int ivx_dev_maskren_render(const uint8_t *mask, const uint8_t *cells, const int64_t shape[3], const int64_t strides[3],
                           int apron, int apron_value, int iso, const float *table, const uint32_t *prefix,
                           const ivx_volren_params *p, void *out, float *depth, uint64_t *stats, void *stream);
int ivx_mask_preview(const uint8_t *matrix, const int64_t shape[3], const int64_t strides[3], int iso, const float *table,
                     const uint32_t *prefix, const ivx_volren_params *p, void *out, float *depth);

/* ------------------------------------------------------------------------------------------------
 * 3-D scene: the ray-cast field, the surfaces and the three slice planes in ONE picture, every surface and plane fragment
 *   blended at its depth inside the field's front-to-back composite (the reference's 3-D viewer with
 *   IntermixIntersectingGeometryOn, invesalius/data/volume.py:644, volume_mask.py:52, and viewer_volume.SlicePlane).
 *   The contract is DESIGN.md section 7r (S1 - S3); PARITY UNPINNED vs VTK's renderer (not installable here).
 * The field (field_kind): IVX_SCENE_FIELD_NONE; IVX_SCENE_FIELD_IMAGE, the prepared uint16 field and uint16 cells of
 *   ivx_dev_volren_render (strides, apron, apron_value unused); IVX_SCENE_FIELD_MASK, the uint8 mask and uint8 cells of
 *   ivx_dev_maskren_render's composite mode with its strides and apron (n_table >= 257, no clip plane, and `p->origin` moved
 *   by (sx, -sy, sz) as there).  p->mip must be 0.  table / prefix as for those calls.
 * The surfaces: `layers` with the keys of ivx_dev_surface_raster for `cam`, whose viewport must be p's.
 * The planes: at most IVX_SCENE_MAX_PLANES, one per orientation; `picture` is dense RGB8 of h rows x w columns as
 *   get_image_slice lays a slice out (AXIAL y x x, CORONAL z x x, SAGITAL z x y); the plane lies at image slice `slice` and is
 *   cut to the rectangle of the voxel centres 0 .. w - 1, 0 .. h - 1; unlit, blended with `opacity`.
 * ivx_dev_scene_render  device pointers (layers, cam, planes, p: host structs that hold device pointers); only enqueues.
 *                       out: height x width x 4 float32, or uint8 with p->out_u8; stats as for ivx_dev_volren_render.
 * ivx_scene_render      host form: `field` is the int16 image (shift, nsmooth as for ivx_volume_render) or the padded uint8
 *                       matrix (as for ivx_mask_preview) with `strides`; the layers' arrays and the planes' pictures are host
 *                       pointers (the layers' keys are ignored).  Uploads, prepares, builds the cells, rasters and renders.
 * Errors (IVX_EINVAL): more than 8 layers, more than 3 planes or a repeated orientation, p->mip, a viewport of `cam` that is
 *   not p's.
 * ---------------------------------------------------------------------------------------------- */
#define IVX_SCENE_FIELD_NONE 0
#define IVX_SCENE_FIELD_IMAGE 1
#define IVX_SCENE_FIELD_MASK 2
#define IVX_SCENE_MAX_PLANES 3
#define IVX_SCENE_AXIAL 0
#define IVX_SCENE_CORONAL 1
#define IVX_SCENE_SAGITAL 2
typedef struct ivx_scene_plane {
    const uint8_t *picture; /* h x w x 3 bytes, dense */
    int32_t h, w;
    int32_t orientation; /* IVX_SCENE_AXIAL .. IVX_SCENE_SAGITAL */
    int32_t slice;       /* image slice number n: world z = n sz / y = -n sy / x = n sx */
    float opacity;
    int32_t reserved;
} ivx_scene_plane;
int ivx_dev_scene_render(int field_kind, const void *field, const void *cells, const int64_t shape[3],
                         const int64_t strides[3], int apron, int apron_value, const float *table, const uint32_t *prefix,
                         const ivx_surface_layer *layers, int nlayers, const ivx_surface_camera *cam, int interpolation,
                         const ivx_scene_plane *planes, int nplanes, const ivx_volren_params *p, void *out, uint64_t *stats,
                         void *stream);
int ivx_scene_render(int field_kind, const void *field, const int64_t shape[3], const int64_t strides[3], int shift,
                     int nsmooth, const float *table, const uint32_t *prefix, const ivx_surface_layer *layers, int nlayers,
                     const ivx_surface_camera *cam, int interpolation, const ivx_scene_plane *planes, int nplanes,
                     const ivx_volren_params *p, void *out);

/* ------------------------------------------------------------------------------------------------
 * slice display: window/level, colour tables, mask and aux overlays, blend -- one launch per picture
 *   replaces Slice.GetSlices (invesalius/data/slice_.py:746-830) with do_ww_wl, do_colour_image, do_colour_mask,
 *   do_custom_colour and do_blend (:1656-1695, :1771-1873).  The arithmetic of VTK's filters is stated as rules R1 - R7 in
 *   DESIGN.md section 7l and csrc/slice_show_math.h; the byte tables come from invesalius3_amd/slice_display.py.
 * Operands are 2-D views of h x w pixels with byte strides of any sign (row, element):
 *   image  what image_kind says: int16 or float64 values (the window/level stage must be on), or a picture's bytes --
 *          IVX_SHOW_U8 one grey byte per pixel (an element stride of 3 reads the first channel of an RGB picture),
 *          IVX_SHOW_RGB8 three bytes per pixel (the window/level stage must be off)
 *   mask   uint8 bytes coloured through table 1 when IVX_SHOW_MASK is on, else RGBA pixels (4 bytes each); may be null
 *   aux    the same with IVX_SHOW_AUX and table 2; may be null
 *   out    dense h x w x out_channels bytes.  3: the picture.  4: the one overlay given, coloured and not blended (the
 *          reference's do_colour_mask / do_custom_colour seams); IVX_SHOW_BLEND must then be off.
 * tables: 3 x 256 RGBA bytes (image table: the HSV table of R2, or the plist table of R3; mask table R5; aux table R6), then
 *   n_nodes float64 node values (ascending) and 3 n_nodes float64 colours c / 255 (R4); 8-byte aligned.
 * ivx_dev_slice_show  device pointers; only enqueues on `stream`.
 * ivx_slice_show      host pointers.  Views of a registered array (ivx_host_register) are gathered from its mirror: nothing
 *                     but the tables goes host -> device and exactly h * w * out_channels bytes come back; otherwise the
 *                     views alone are uploaded.
 * ---------------------------------------------------------------------------------------------- */
#define IVX_SHOW_WWWL 1
#define IVX_SHOW_COLOUR 2
#define IVX_SHOW_MASK 4
#define IVX_SHOW_AUX 8
#define IVX_SHOW_BLEND 16
#define IVX_SHOW_I16 0
#define IVX_SHOW_F64 1
#define IVX_SHOW_U8 2
#define IVX_SHOW_RGB8 3
#define IVX_SHOW_MAX_NODES 256
typedef struct ivx_slice_show_params {
    int32_t image_kind;   /* IVX_SHOW_I16 .. IVX_SHOW_RGB8 */
    int32_t mode;         /* 0 OTHER (R1 + R2), 1 PLIST (R3), 2 WIDGET (R4) */
    int32_t stages;       /* IVX_SHOW_* bits */
    int32_t n_nodes;      /* WIDGET: 1 .. IVX_SHOW_MAX_NODES */
    int32_t aux_max;      /* largest key of the aux colour dict (R6) */
    int32_t out_channels; /* 3 or 4 */
    double window_width, window_level;
    double table_min, table_max; /* R2: get_LUT_value_255((image min, image max), ww, wl) */
} ivx_slice_show_params;
int ivx_slice_show_tables_bytes(int n_nodes, size_t *nbytes);
int ivx_dev_slice_show(const void *image, int64_t image_row_stride, int64_t image_elem_stride, const uint8_t *mask,
                       int64_t mask_row_stride, int64_t mask_elem_stride, const uint8_t *aux, int64_t aux_row_stride,
                       int64_t aux_elem_stride, int64_t h, int64_t w, const ivx_slice_show_params *p, const void *tables,
                       uint8_t *out, void *stream);
int ivx_slice_show(const void *image, int64_t image_row_stride, int64_t image_elem_stride, const uint8_t *mask,
                   int64_t mask_row_stride, int64_t mask_elem_stride, const uint8_t *aux, int64_t aux_row_stride,
                   int64_t aux_elem_stride, int64_t h, int64_t w, const ivx_slice_show_params *p, const void *tables,
                   uint8_t *out);

/* ------------------------------------------------------------------------------------------------
 * density measures: the statistics of the pixels an ellipse or a polygon selects on a slice -- a batch of R regions per launch
 *   replaces CircleDensityMeasure.calc_density and PolygonDensityMeasure.calc_density (invesalius/data/measures.py:2019-2107,
 *   2229-2319).  Which pixels a region selects is stated as rules E and P in DESIGN.md section 7o and csrc/density_roi_math.h.
 * A region reads a 2-D view of h x w int16 pixels with byte strides of any sign (row, element), the convention of
 * ivx_dev_slice_show: one form serves the three orientations of a volume and a plain 2-D array.
 *   ellipse  pixel (row j, column i) is selected iff (i sx - cx)^2 / a2 + (j sy - cy)^2 / b2 <= 1 in float64; a2 and b2 are
 *            the squares as the caller computes them (Python's a ** 2)
 *   polygon  n_points points (x, y) in pixel units, from index first_point of the call's points block; pixel (j, i) is
 *            selected iff its centre (i + 0.5, j + 0.5) is inside by the odd-even crossing test of ivx_polygon2mask.  Fewer
 *            than 3 points select nothing; more than IVX_ROI_MAX_POINTS (they sit in LDS) is IVX_EINVAL.
 * The library fills x0 .. n_blocks of its own copy of every descriptor (the box of pixels the region can select, clipped to
 * the slice and one pixel wider than the bound; the workgroups' prefix sums); what the caller puts there is ignored.
 * records: five 8-byte integers per region -- cnt, s1 (sum), s2 (sum of squares), lo, hi; lo = hi = 0 when cnt is 0.
 * ivx_dev_roi_density  the images, points_dev and records are device pointers, the descriptors host memory (read before the
 *                      call returns); points_host: the same points for the polygons' boxes, or NULL (whole slices are then
 *                      scanned).  One memset and one launch on `stream`, whatever n_rois is; only enqueues.
 * ivx_roi_density      host pointers.  Regions on a registered array (ivx_host_register) are read from its mirror in place:
 *                      nothing but descriptors and points goes host -> device; otherwise the boxes alone are uploaded.
 *                      Exactly IVX_ROI_RECORD_BYTES * n_rois bytes come back.
 * ---------------------------------------------------------------------------------------------- */
#define IVX_ROI_ELLIPSE 0
#define IVX_ROI_POLYGON 1
#define IVX_ROI_MAX_POINTS 2048 /* 32 KB of LDS */
#define IVX_ROI_RECORD_BYTES 40
typedef struct ivx_roi {
    const void *image;               /* element [0][0] of the int16 view */
    int64_t row_stride, elem_stride; /* bytes, any sign */
    int64_t h, w;
    int32_t kind;     /* IVX_ROI_ELLIPSE, IVX_ROI_POLYGON */
    int32_t n_points; /* polygon */
    int64_t first_point;
    double sx, sy, cx, cy, a2, b2;   /* ellipse */
    int64_t x0, y0, x1, y1;          /* filled by the library: columns [x0, x1), rows [y0, y1) */
    int64_t first_block, n_blocks;   /* filled by the library */
} ivx_roi;
int ivx_dev_roi_density(const ivx_roi *rois, int64_t n_rois, const double *points_host, const double *points_dev, int64_t n_points,
                        int64_t *records, void *stream);
int ivx_roi_density(const ivx_roi *rois, int64_t n_rois, const double *points, int64_t n_points, int64_t *records);

/* ------------------------------------------------------------------------------------------------
 * The 3-D mask editor (csrc/k_mask3d.hip, csrc/mask3d_math.h): Mask3DEditorState of
 * invesalius/data/mask3d_editor_state.py on mask_cut.rs, brush_mask.rs and polygon_mask.rs, in place on the padded mask matrix.
 * `matrix` is element [0][0][0] of the (d+1, h+1, w+1) uint8 matrix, `shape` its interior (d, h, w), `strides` its byte
 * strides, which must be the dense ((h+1)(w+1), w+1, 1).  (With the strides (h w, w, 1) `matrix` is a dense block of the voxels
 * alone, as a DeviceVolume keeps its mask: cut and brush stroke take that too, with d plane flags.)  Row 0 of every axis (the slice flags) is never read as a voxel and
 * never written.  edit_mode: 0 include, 1 exclude.  `plane_flags`: d+1 bytes, one per matrix[z]; a kernel stores 1 where it
 * changed a byte of that plane and never stores 0 (the caller clears them).
 * ivx_dev_m3e_filter         out[y * w + x] = OR_k polygon2mask_rs((w, h), polygon k)[x][y], inverted for include: an (h, w)
 *                            byte image.  points_dev: all polygons' display points (x, y) as float64, polygon k being points
 *                            offsets_dev[k] .. offsets_dev[k+1]-1 (n_polygons + 1 int64 offsets, device).  Any number of
 *                            points: they are read from global memory, there is no cap.  n_polygons == 0: all 0 (all 1).
 * ivx_dev_m3e_cut            mask_cut on the interior; `filter` is the dense (mh, mw) byte image, m / mv 16 doubles each, row-major
 *                            (host).  One launch; no staging copy.
 * ivx_dev_m3e_brush_stroke   n_centres dabs of brush_mask_rs with one radius, equal to the calls made one after another.
 *                            centres: (x, y, z) float64 in the kernel's coordinates, given twice: centres_host for the boxes,
 *                            centres_dev for the kernel.  `orig`: a padded matrix of the same strides, or NULL.  One launch per
 *                            ivx_m3e_brush_capacity() centres, over the union of their clipped boxes.  Any edit_mode but 0 and 1
 *                            touches nothing.
 * ivx_dev_m3e_equal          *equal = the n bytes at a and b are the same (one int comes back; waits for `stream`)
 * The host forms take the host matrix.  On a registered matrix (ivx_host_register) they work in its mirror and copy the runs of
 * changed planes mirror -> host, so both hold the same bytes afterwards; any other matrix is staged once, up, and its changed
 * planes come down.  ivx_m3e_cut takes the filter as an (mh, mw) byte image, or -- with filter == NULL -- the polygons, from
 * which it makes the (mh, mw) filter on the device.  *planes_written: the planes copied to the host.
 * ---------------------------------------------------------------------------------------------- */
int ivx_m3e_brush_capacity(void);
int ivx_dev_m3e_filter(int64_t w, int64_t h, const double *points_dev, const int64_t *offsets_dev, int64_t n_polygons, int edit_mode,
                       uint8_t *out, void *stream);
int ivx_dev_m3e_cut(uint8_t *matrix, const int64_t shape[3], const int64_t strides[3], const double spacing[3], double max_depth,
                    const uint8_t *filter, int64_t mh, int64_t mw, const double *m, const double *mv, int edit_mode,
                    uint8_t *plane_flags, void *stream);
int ivx_dev_m3e_brush_stroke(uint8_t *matrix, const uint8_t *orig, const int64_t shape[3], const int64_t strides[3],
                             const double spacing[3], const double *centres_host, const double *centres_dev, int64_t n_centres,
                             double radius, int edit_mode, uint8_t *plane_flags, void *stream);
int ivx_dev_m3e_equal(const uint8_t *a, const uint8_t *b, int64_t n, int *equal, void *stream);
/* matrix[1:, 1:, 1:] = src[1:, 1:, 1:] (update_views:262) for a padded device block `src` of the matrix's shape; only bytes that
 * differ are stored.  The host form follows the rules of the other host forms. */
int ivx_dev_m3e_apply(uint8_t *matrix, const uint8_t *src, const int64_t shape[3], const int64_t strides[3], uint8_t *plane_flags,
                      void *stream);
int ivx_m3e_apply(uint8_t *matrix, const uint8_t *src_dev, const int64_t shape[3], const int64_t strides[3], int64_t *planes_written);
/* Mask.modified(all_volume=True): matrix[0] = matrix[:, 0, :] = matrix[:, :, 0] = 1, by the CPU on the host and by a kernel in a
 * registered matrix's mirror; no byte crosses the link. */
int ivx_m3e_flag_planes(uint8_t *matrix, const int64_t shape[3], const int64_t strides[3]);
int ivx_m3e_filter(int64_t w, int64_t h, const double *points, const int64_t *offsets, int64_t n_polygons, int edit_mode, uint8_t *out);
int ivx_m3e_cut(uint8_t *matrix, const int64_t shape[3], const int64_t strides[3], const double spacing[3], double max_depth,
                const uint8_t *filter, int64_t mh, int64_t mw, const double *points, const int64_t *offsets, int64_t n_polygons,
                const double *m, const double *mv, int edit_mode, int64_t *planes_written);
int ivx_m3e_brush_stroke(uint8_t *matrix, const uint8_t *orig, const int64_t shape[3], const int64_t strides[3], const double spacing[3],
                         const double *centres, int64_t n_centres, double radius, int edit_mode, int64_t *planes_written);

/* ------------------------------------------------------------------------------------------------
 * bench / test input made in HBM (no reference counterpart): a CT-like int16 phantom -- six Gaussian blobs + sinusoid +
 * hashed N(0,25) noise, clipped to [-1024, 3071] -- for the slices [z0, z0 + dz) of a z_total-slice volume; deterministic
 * in (seed, global voxel index), so slabs made by different ranks tile the whole volume.  centres_zyx_sigma: 6 x (cz, cy,
 * cx, sigma) in normalised coordinates.  Used by bench.py --config sharded2048 (BASELINE configs[3]).
 * ---------------------------------------------------------------------------------------------- */
int ivx_dev_synth_volume(int16_t *out, int64_t dz, int64_t dy, int64_t dx, int64_t z0, int64_t z_total, uint32_t seed,
                         const float centres_zyx_sigma[24], void *stream);

/* ------------------------------------------------------------------------------------------------
 * Z-slab communicator: RCCL over xGMI behind the C ABI (one process per GPU).
 *   the reference's decomposition: Z pieces + one overlap slice, invesalius/data/surface.py:1362-1380;
 *   it has no multi-GPU code, so these entry points replace nothing upstream -- they are what the sharded
 *   driver (invesalius3_amd/parallel.py, bench.py --gpus N) binds instead of torch.distributed.
 * librccl.so is dlopen'ed by the first call.  All buffers are DEVICE pointers; every call only enqueues on `stream`.
 *   ivx_comm_unique_id   rank 0 makes the 128-byte id; it reaches the other ranks out of band (a file / env)
 *   ivx_comm_init        collective over all ranks, on the calling process's current device
 *   ivx_comm_exchange    to_down -> rank-1, to_up -> rank+1 and the mirror receives, one group (halo slices, planes)
 *   ivx_comm_exchange_vote   the same followed by an in-place int32 sum all-reduce of `vote` on the same stream
 *   ivx_comm_allreduce   in place; op 0 sum / 1 max / 2 min; IVX_I32 / I64 / F32 / F64 / U8 / I8 (no 16-bit integers)
 *   ivx_comm_allgather   recv = world * nbytes, rank order;   ivx_comm_bcast / send / recv: raw bytes
 * ---------------------------------------------------------------------------------------------- */
int ivx_comm_unique_id(uint8_t id[128]);
int ivx_comm_init(const uint8_t id[128], int rank, int world, void **comm);
int ivx_comm_destroy(void *comm);
int ivx_comm_rank(const void *comm, int *rank, int *world);
int ivx_comm_exchange(void *comm, const void *to_down, void *from_down, const void *to_up, void *from_up, size_t nbytes,
                      void *stream);
int ivx_comm_exchange_vote(void *comm, const void *to_down, void *from_down, const void *to_up, void *from_up,
                           size_t nbytes, int32_t *vote, int nvote, void *stream);
int ivx_comm_allreduce(void *comm, void *buf, size_t count, int dtype, int op, void *stream);
int ivx_comm_allgather(void *comm, const void *send, void *recv, size_t nbytes, void *stream);
int ivx_comm_bcast(void *comm, void *buf, size_t nbytes, int root, void *stream);
int ivx_comm_send(void *comm, const void *buf, size_t nbytes, int peer, void *stream);
int ivx_comm_recv(void *comm, void *buf, size_t nbytes, int peer, void *stream);
/* Every entry point above once, on 4 KB buffers, checked against the analytic answer; the error names the collective that
 * failed.  Collective: every rank calls it.  At world 1, where the entry points never reach RCCL, it drives RCCL directly
 * on the one-rank communicator (all-reduce, all-gather, broadcast, a grouped send + receive to itself). */
int ivx_comm_selftest(void *comm, void *stream);

/* ------------------------------------------------------------------------------------------------
 * surface import: a triangle soup (what an STL file holds) to a welded indexed mesh (csrc/k_meshweld.hip)
 *   replaces vtkSTLReader's point merge (vtkMergePoints::InsertUniquePoint per corner in file order) behind
 *   Surface.CreateSurfaceFromFile, and ConvertPolydataToInv's transform (invesalius/data/surface.py:625-870).
 * Weld: corners whose three float32 coordinates compare equal as numbers are one point (-0.0 == +0.0); the stored point is the
 * first occurrence with its own bits; ids by first occurrence in corner order 3 t + c; a facet whose ids are not pairwise
 * different is dropped afterwards (its points stay), the kept facets in order.  A coordinate that is not finite is IVX_EDOM.
 * Limits: 3 T <= 2^31 - 1 (IVX_EDOM before any launch); the table has the power of two >= 2 * 3 T slots.
 *   ivx_mesh_weld_slots   that slot count (host only, no device needed)
 *   ivx_mesh_weld_bytes   the scratch ivx_dev_mesh_weld needs for T triangles
 *   ivx_dev_mesh_weld     soup (3 T, 3) float32 -> verts_out (room for 3 T points), faces_out (room for T facets) and the
 *                         IVX_WELD_COUNT_WORDS uint32 words of counts_out, all device memory; queue-only.  The caller downloads
 *                         the words: IVX_WELD_OVERRUN set is IVX_EINTERNAL, IVX_WELD_NONFINITE set is IVX_EDOM.
 *   ivx_dev_stl_unpack    the bytes of a binary STL of T records (84 + 50 T of them, at a 16-byte aligned device address) ->
 *                         the soup; *flag (device, zeroed by the caller) gets bit 0 when a coordinate is not finite
 *   ivx_dev_mesh_transform_points  out[i] = float32(((m[r][0] x + m[r][1] y) + m[r][2] z) + m[r][3]) in float64, rows 0..2 of
 *                         the row-major 4 x 4 `m16` (host memory); out may be verts
 * Host forms take host pointers (verts_out: room for 3 T points, faces_out: T facets, counts: IVX_WELD_COUNT_WORDS int64);
 * ivx_mesh_stl_weld takes the whole file (nbytes must be 84 + 50 * its count: IVX_EDOM).
 * ---------------------------------------------------------------------------------------------- */
#define IVX_WELD_COUNT_WORDS 32
#define IVX_WELD_VERTS 0      /* points of the welded mesh */
#define IVX_WELD_KEPT 1       /* facets kept */
#define IVX_WELD_DROPPED 2    /* degenerate facets dropped */
#define IVX_WELD_OVERRUN 3    /* a probe walked the whole table */
#define IVX_WELD_NONFINITE 4  /* a coordinate was not finite */
#define IVX_WELD_MAX_PROBE 5  /* the longest walk, in slots past the home slot */
#define IVX_WELD_LOG2_SLOTS 6 /* log2 of the table's slot count */
#define IVX_WELD_HIST 8       /* 16 words: corners by walk length 0, 1, 2-3, 4-7, ..., >= 16384 */
int ivx_mesh_weld_slots(int64_t n_corners, uint64_t *slots);
int ivx_mesh_weld_bytes(int64_t ntris, size_t *bytes);
int ivx_dev_mesh_weld(const float *soup, int64_t ntris, void *scratch, float *verts_out, int32_t *faces_out,
                      uint32_t *counts_out, void *stream);
int ivx_dev_stl_unpack(const uint8_t *bytes, int64_t ntris, float *soup_out, uint32_t *flag, void *stream);
int ivx_dev_mesh_transform_points(const float *verts, int64_t nverts, const double *m16, float *out, void *stream);
int ivx_mesh_weld(const float *soup, int64_t ntris, float *verts_out, int32_t *faces_out, int64_t *counts);
int ivx_mesh_stl_weld(const uint8_t *file_bytes, size_t nbytes, float *verts_out, int32_t *faces_out, int64_t *counts);
int ivx_mesh_transform_points(const float *verts, int64_t nverts, const double *m16, float *out);

#ifdef __cplusplus
}
#endif
#endif /* IVX_H */

/* bsmi_io.h -- C ABI of the volume I/O half of libbsmi.so: Zarr v2 chunk codecs and threaded
 * chunk-file decode / encode (host only, no device work).
 *
 * Replaces what the reference gets from zarr-python + numcodecs underneath
 * funlib.persistence.open_ds / prepare_ds (paths relative to /root/reference/bootstrapper:
 * predict.py:169-178, post/watershed.py:319-330, post/blockwise/watershed_frags.py:61-98,
 * data/volumes.py:14-19): the `compressor` entry of a `.zarray` selects one bsmi_codec.
 * Same conventions as bsmi.h: 0 on success, negative on failure, message from
 * bsmi_last_error() (per calling thread).
 */
#ifndef BSMI_IO_H
#define BSMI_IO_H

#include <stddef.h>
#include <stdint.h>

#include "bsmi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bsmi_codec.id: the numcodecs codec of `.zarray["compressor"]["id"]` */
#define BSMI_CODEC_RAW 0   /* "compressor": null                                       */
#define BSMI_CODEC_ZLIB 1  /* {"id": "zlib", "level": L}                               */
#define BSMI_CODEC_GZIP 2  /* {"id": "gzip", "level": L}                               */
#define BSMI_CODEC_ZSTD 3  /* {"id": "zstd", "level": L}: one zstd frame               */
#define BSMI_CODEC_LZ4 4   /* {"id": "lz4", "acceleration": A}: u32 size + LZ4 block   */
#define BSMI_CODEC_BLOSC 5 /* {"id": "blosc", "cname", "clevel", "shuffle", "blocksize"} */

/* bsmi_codec.cname for BSMI_CODEC_BLOSC when encoding (decoding reads it from the frame and
 * also takes lz4hc and blosclz frames) */
#define BSMI_BLOSC_LZ4 1
#define BSMI_BLOSC_ZLIB 3
#define BSMI_BLOSC_ZSTD 4

/* status of one chunk in bsmi_chunks_read: the file does not exist (zarr: fill_value chunk) */
#define BSMI_CHUNK_MISSING 1

typedef struct bsmi_codec {
  int32_t id;        /* BSMI_CODEC_*                                                    */
  int32_t level;     /* zlib / gzip / zstd level, blosc clevel (0..9)                    */
  int32_t cname;     /* blosc: BSMI_BLOSC_*                                              */
  int32_t shuffle;   /* blosc: 0 none, 1 byte shuffle, 2 bit shuffle (numcodecs' -1 "auto"
                        is resolved by the caller: bit shuffle for 1-byte items)         */
  int32_t typesize;  /* blosc: item size of the array's dtype                            */
  int32_t blocksize; /* blosc: 0 = library default                                       */
} bsmi_codec;

/* Upper bound of the encoded size of n bytes (numcodecs Codec.encode allocates the same way). */
size_t bsmi_codec_bound(const bsmi_codec *codec, size_t n);

/* numcodecs Codec.decode(buf, out=dst): decode one chunk into dst (capacity cap bytes);
 * *out_len = decoded bytes.  Fails if the chunk is corrupt or larger than cap.            */
int bsmi_codec_decode(const bsmi_codec *codec, const void *src, size_t n, void *dst, size_t cap, size_t *out_len);

/* numcodecs Codec.encode(buf): encode n bytes into dst (cap >= bsmi_codec_bound).          */
int bsmi_codec_encode(const bsmi_codec *codec, const void *src, size_t n, void *dst, size_t cap, size_t *out_len);

/* zarr.Array.__getitem__ over a set of chunks (zarr/core.py _chunk_getitems -> store read +
 * Codec.decode per chunk): read and decode n chunk files on `threads` host threads.
 * status[i] = BSMI_OK, BSMI_CHUNK_MISSING (no such file: the caller fills with fill_value) or a
 * negative code; lens[i] = decoded bytes.  Returns the first failure, if any.               */
int bsmi_chunks_read(const bsmi_codec *codec, int n, const char *const *paths, void *const *dsts, const size_t *caps,
                     size_t *lens, int *status, int threads);

/* zarr.Array.__setitem__ over whole chunks (_chunk_setitems -> Codec.encode + store write):
 * encode and write n chunk files (write to a temporary name, then rename) on `threads` threads. */
int bsmi_chunks_write(const bsmi_codec *codec, int n, const char *const *paths, const void *const *srcs,
                      const size_t *sizes, int *status, int threads);

/* One chunk <-> one region of a strided host array (arrays of up to 4 axes; fewer: leading axes of length 1).  What zarr-python's
 * _chunk_getitems / _chunk_setitems do chunk by chunk in the caller's interpreter (decode into a chunk-sized array, then copy the
 * overlap; reference reads: funlib.persistence Array.to_ndarray under post/blockwise/watershed_frags.py:196-201, writes:
 * `array[roi] = data` at :222-226) happens here inside the worker thread that decodes / encodes the chunk. */
typedef struct bsmi_chunk_copy {
  const char *path;          /* the chunk's file                                                               */
  void *base;                /* host address of the region's first element                                     */
  int64_t start[4];          /* first element of the region inside the chunk, per axis                         */
  int64_t extent[4];         /* elements per axis (>= 1)                                                       */
  int64_t stride[4];         /* byte strides of the host array; stride[3] must equal the item size             */
  int32_t read_modify_write; /* write: the region covers only part of the chunk's valid extent -- keep the rest of
                                what the file holds (0: the rest becomes the fill value)                       */
  int32_t reserved;
} bsmi_chunk_copy;

/* Read n regions: decode each chunk (Blosc: only the blocks up to the region's last byte -- reading three of six channels of an
 * affinity chunk decodes half of it) and copy the region's rows into the host array.  A missing file fills the region with
 * fill_value (itemsize bytes; NULL = zeros) and sets status[i] = BSMI_CHUNK_MISSING. */
int bsmi_chunks_read_into(const bsmi_codec *codec, int n, const bsmi_chunk_copy *copies, const int64_t chunk_shape[4],
                          int itemsize, const void *fill_value, int *status, int threads);
/* Write n regions: gather the rows from the host array into a chunk image (the rest fill_value, or the file's old content
 * when read_modify_write), encode, write to a temporary name, rename. */
int bsmi_chunks_write_from(const bsmi_codec *codec, int n, const bsmi_chunk_copy *copies, const int64_t chunk_shape[4],
                           int itemsize, const void *fill_value, int *status, int threads);

/* Blosc frames of a DEVICE-resident volume of 8-byte items (fragment / segment ids), made on the device (csrc/blosc_dev.hip):
 * what `array[roi] = data` on a Zarr dataset with zarr-python's default compressor produces (Blosc-1, lz4, byte shuffle, 256 KiB
 * split blocks; reference post/watershed.py:319-354, post/blockwise/watershed_frags.py:222-226) without taking the 8 bytes per
 * voxel across PCIe and through the host's encoder: only the frames, a few percent of the volume, leave the device.
 * src_dev[z * stride_z + y * stride_y + x] (strides in elements) is the volume; chunk i starts at origins[3 i ..] (voxels,
 * relative to src_dev), extents[3 i ..] <= chunk_shape of it exist (the rest of the chunk is fill value 0: chunks that overhang
 * the array).  chunk_shape: whole 256 KiB blocks (chunk bytes a multiple of 262 144, e.g. 128^3 or 8 x 64 x 64 items).
 * frames_dev: n_chunks slots of slot_bytes >= bsmi_blosc_dev_frame_bound(chunk bytes); frame_sizes_dev[i] = bytes of frame i.
 * scratch_dev: bsmi_blosc_dev_scratch_bytes(n_chunks, chunk bytes).  Asynchronous on `stream`; origins / extents are host arrays
 * that must stay valid until the stream has passed the call.  Any Blosc-1 reader decodes the frames (the LZ4 blocks use matches
 * at offset 1 only; liblz4 would pack label volumes about twice as tight). */
size_t bsmi_blosc_dev_frame_bound(size_t chunk_bytes);
size_t bsmi_blosc_dev_scratch_bytes(int n_chunks, size_t chunk_bytes);
int bsmi_blosc_encode_dev_u64(int device, const uint64_t *src_dev, int64_t stride_z, int64_t stride_y, int n_chunks,
                              const int64_t *origins, const int64_t *extents, const int64_t chunk_shape[3], void *scratch_dev,
                              size_t scratch_bytes, void *frames_dev, size_t slot_bytes, uint32_t *frame_sizes_dev, void *stream);

/* Blosc frames of a DEVICE-resident array of 1-byte items (the affinity / LSD chunks of `bs predict`), made on the device
 * (csrc/blosc_dev_u8.hip): Blosc-1, lz4 format, typesize 1, blocks of 32 KiB not split (flags 0x30; the last block may be short,
 * a frame that would not shrink is stored).  The LZ4 blocks hold matches at offset 1 (runs) and at the distances a 4096-entry
 * table finds; the rule is written out in blosc_dev_u8.hip and restated in tests/blosc_u8_ref.py, and the frames are byte-equal
 * to that restatement.  Any Blosc-1 reader decodes them.
 * src_dev[c * strides[0] + z * strides[1] + y * strides[2] + x] (strides in elements, x contiguous) is the array, chunks are
 * (C, Z, Y, X) -- a 3-D array has C = 1; chunk i starts at origins[4 i ..] (relative to src_dev), extents[4 i ..] <= chunk_shape
 * of it exist, the rest of the chunk is fill value 0.  A chunk holds 1 byte ... 1024 blocks (32 MiB); larger ones, null arguments,
 * extents outside 1 ... chunk_shape, negative origins and slots or scratch below the two bounds give BSMI_ERR_INVALID.
 * frames_dev: n_chunks slots of slot_bytes >= bsmi_blosc_dev_u8_frame_bound(chunk bytes); frame_sizes_dev[i] = bytes of frame i;
 * scratch_dev: bsmi_blosc_dev_u8_scratch_bytes(n_chunks, chunk bytes).  Asynchronous on `stream`.  origins, extents, strides and
 * chunk_shape are read before the call returns (they travel in launch arguments): the caller may free them at once. */
size_t bsmi_blosc_dev_u8_frame_bound(size_t chunk_bytes);
size_t bsmi_blosc_dev_u8_scratch_bytes(int n_chunks, size_t chunk_bytes);
int bsmi_blosc_encode_dev_u8(int device, const uint8_t *src_dev, const int64_t strides[3], int n_chunks, const int64_t *origins,
                             const int64_t *extents, const int64_t chunk_shape[4], void *scratch_dev, size_t scratch_bytes,
                             void *frames_dev, size_t slot_bytes, uint32_t *frame_sizes_dev, void *stream);

/* The region adjacency graph of a segmented volume as an SQLite file (the `db` table of the reference's segment config,
 * post/watershed.py:100-117; nodes as post/blockwise/watershed_frags.py:230-246 writes them, edges with their merge scores
 * as waterz_agglom.py:165-170): tables nodes(id PRIMARY KEY, z, y, x, size) and edges(u, v, merge_score, PRIMARY KEY (u, v)),
 * a NaN score stored as NULL (never merged).  positions [n_nodes][3] world units, edges [n_edges][2].  libsqlite3.so.0 is
 * loaded at run time; BSMI_ERR_MISSING if it cannot be. */
int bsmi_rag_write_sqlite(const char *path, uint64_t n_nodes, const uint64_t *ids, const double *positions, const int64_t *sizes,
                          uint64_t n_edges, const uint64_t *edges, const float *scores);

#ifdef __cplusplus
}
#endif
#endif /* BSMI_IO_H */

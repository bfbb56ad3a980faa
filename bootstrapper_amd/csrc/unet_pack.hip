// Unit lists and weight images of the U-Net engine: what bsmi_unet_finalize builds from the host copies of the weights -- per
// ConvPass stage the K-step units of its implicit GEMM (build_entries) and the packed image of every form the stage may take
// (pack_conv: the gather / raster-halo kernels of each precision; pack_wino, pack_h16: the split-bf16 mode's Winograd and
// halo-resident forms) -- and their release.
#include <cstdlib>
#include <cstring>

#include "unet_internal.h"

#include "dev_guard.h"  // last: routes hipMalloc / hipFree through the guarded allocator (BSMI_GUARD_MB)

namespace bsmi {

int esize(int prec) { return prec == BSMI_PREC_F32 ? 4 : 2; }
int ksplit(int prec) { return prec == BSMI_PREC_BF16X3 ? 3 : 1; }  // listed form; PackedConv::ks holds the layer's own value
int bke(int prec) { return kStepRowBytes / esize(prec); }
int sube(int prec) { return 32 / esize(prec); }

// v as a bf16 pair: its high part and what that leaves
static inline void split_bf16(float v, uint16_t& hi, uint16_t& lo) {
  hi = host_f32_to_bf16(v);
  lo = host_f32_to_bf16(v - host_bf16_to_f32(hi));
}

// The device images of a packed form, freed and forgotten: before a stage is packed again (bsmi_unet_finalize) and when the
// handle goes (bsmi_unet_destroy).  Every device pointer of a Packed* struct is listed here and nowhere else.
template <class T>
static void release_image(T*& w) {
  if (w) (void)hipFree(w);
  w = nullptr;
}
void release(PackedConv& pc) {
  release_image(pc.w);
  release_image(pc.bias);
  pc.ready = false;
}
void release(PackedWino& pw) {
  release_image(pw.w);
  release_image(pw.res_w);
  for (int part = 0; part < 2; ++part) release_image(pw.res_part_w[part]);
  release_image(pw.skip_w);
  release_image(pw.below_w);
  pw.below_ready = false;
  pw.ready = false;
}
void release(PackedH16& ph) {
  release_image(ph.w);
  ph.ready = false;
}

// Build the unit list of stage `ci` of a ConvPass.  kUnitsPerStep consecutive entries = one
// K-step.  Order: for every source slot, 32-channel chunk major with the kernel taps inside (one
// tap x 32 channels per K-step, i.e. 64 contiguous bytes per gathered row; a 16-channel tensor
// packs two taps per K-step), then, for the last stage, the cropped 1x1x1 residual in 32-channel
// chunks.  Each (slot, 32-channel chunk) is also one PackPhase:
// LONG = all kernel taps of the chunk, SHORT = its residual tap.
void build_entries(const PassSite& p, int ci, int prec, std::vector<PackEntry>& out, std::vector<PackPhase>* phases_out) {
  const int SUB = sube(prec);
  const bool last = ci == p.nconv - 1;
  std::vector<PackPhase> phases;
  auto close_phase = [&](PackPhase ph) {
    while ((out.size() - ph.first_unit) % kUnitsPerStep) out.push_back(PackEntry{ph.slot, 0, 0, 0, 0, 0, 0, 0, 0, true, (int)phases.size()});
    ph.nunits = (int)out.size() - ph.first_unit;
    phases.push_back(ph);
  };
  auto add_taps = [&](int slot, const int* k, int cin_base, int creal) {
    const int cpad = round_up(creal, kChanPad);
    if (cpad == SUB) {
      // a voxel is one 32-byte unit: a K-step takes two x-adjacent taps (dx, dx+1), which are 64
      // contiguous bytes of the channels-last tensor (conv_rh.hip reads them as one halo row)
      PackPhase ph{slot, 0, 0, (int)out.size(), 0};
      for (int z = 0; z < k[0]; ++z)
        for (int y = 0; y < k[1]; ++y)
          for (int x = 0; x < k[2]; x += kUnitsPerStep)
            for (int j = 0; j < kUnitsPerStep; ++j) {
              if (x + j < k[2])
                out.push_back(PackEntry{slot, z, y, x + j, 0, 0, (z * k[1] + y) * k[2] + x + j, cin_base, creal, false, (int)phases.size()});
              else
                out.push_back(PackEntry{slot, 0, 0, 0, 0, 0, 0, 0, 0, true, (int)phases.size()});
            }
      close_phase(ph);
      return;
    }
    for (int c32 = 0; c32 < cpad; c32 += kUnitsPerStep * SUB) {
      PackPhase ph{slot, c32, 0, (int)out.size(), 0};
      for (int z = 0; z < k[0]; ++z)
        for (int y = 0; y < k[1]; ++y)
          for (int x = 0; x < k[2]; ++x) {
            for (int c0 = c32; c0 < std::min(cpad, c32 + kUnitsPerStep * SUB); c0 += SUB)
              out.push_back(PackEntry{slot, z, y, x, c0, 0, (z * k[1] + y) * k[2] + x, cin_base, creal, false, (int)phases.size()});
            while ((out.size() - ph.first_unit) % kUnitsPerStep)  // half chunk: the K-step's second unit is padding
              out.push_back(PackEntry{slot, 0, 0, 0, 0, 0, 0, 0, 0, true, (int)phases.size()});
          }
      close_phase(ph);
    }
  };
  auto add_residual = [&](int slot, const int* crop, int cin_base, int creal) {
    const int cpad = round_up(creal, kChanPad);
    for (int c32 = 0; c32 < cpad; c32 += kUnitsPerStep * SUB) {
      PackPhase ph{slot, c32, 1, (int)out.size(), 0};
      for (int c0 = c32; c0 < std::min(cpad, c32 + kUnitsPerStep * SUB); c0 += SUB)
        out.push_back(PackEntry{slot, crop[0] / 2, crop[1] / 2, crop[2] / 2, c0, 1, 0, cin_base, creal, false, (int)phases.size()});
      close_phase(ph);
    }
  };
  const int* k = p.k[ci];
  if (ci == 0) {
    int base = 0;
    for (int s = 0; s < p.nslots; ++s) {
      add_taps(s, k, base, p.cin[s]);
      base += p.cin[s];
    }
  } else {
    add_taps(0, k, 0, p.cout);
  }
  if (last) {
    int crop[3] = {0, 0, 0};
    for (int i = 0; i < p.nconv; ++i)
      for (int d = 0; d < 3; ++d) crop[d] += p.k[i][d] - 1;
    const int first_slot = ci == 0 ? 0 : 1;
    int base = 0;
    for (int s = 0; s < p.nslots; ++s) {
      add_residual(first_slot + s, crop, base, p.cin[s]);
      base += p.cin[s];
    }
  }
  // an even number of K-steps: the 16x16x32 kernel body is unrolled by two
  if ((out.size() / kUnitsPerStep) % 2)
    for (int j = 0; j < kUnitsPerStep; ++j) out.push_back(PackEntry{0, 0, 0, 0, 0, 0, 0, 0, 0, true, (int)phases.size() - 1});
  if (phases_out) *phases_out = phases;
}

int pack_conv(bsmi_unet* h, PassSite& p, int ci, int prec) {
  PackedConv& pc = p.packed[prec][ci];
  if (pc.ready) return BSMI_OK;
  pc.entries.clear();
  build_entries(p, ci, prec, pc.entries, &pc.phases);
  pc.tile = choose_tile(p.cout);
  pc.Npad = round_up(p.cout, tile_bn(pc.tile));
  const int BKE = bke(prec);
  const bool last = ci == p.nconv - 1;
  const HostWeight& wm = h->weights[p.prefix + ".conv_pass." + std::to_string(2 * ci) + ".weight"];
  const HostWeight& bm = h->weights[p.prefix + ".conv_pass." + std::to_string(2 * ci) + ".bias"];
  const HostWeight& wr = h->weights[p.prefix + ".residual.0.weight"];
  const HostWeight& br = h->weights[p.prefix + ".residual.0.bias"];
  const int64_t cin_m = wm.shape[1], ntap_m = wm.shape[2] * wm.shape[3] * wm.shape[4];
  const int64_t cin_r = wr.shape[1];
  const int SUB = sube(prec);
  // Split mode: logical K-step s becomes the kernel's K-steps 3s (hi activations x hi weights), 3s + 1 (lo
  // activations x hi weights) and 3s + 2 (hi activations x lo weights); the weight image carries a row block for each
  const bool fused = prec == BSMI_PREC_BF16X3 && x3_fused_for(pc.tile);
  const int KS = pc.ks = fused ? 1 : ksplit(prec);
  const size_t nsteps = pc.entries.size() / kUnitsPerStep * KS;
  const size_t nelem = (nsteps * (size_t)pc.Npad + kWeightRowSlack) * BKE;  // slack rows: padded tile loads
  std::vector<float> bias(pc.Npad, 0.f);
  for (int n = 0; n < p.cout; ++n) bias[n] = bm.data[n] + (last ? br.data[n] : 0.f);

  pc.lo_image_bytes = fused ? nelem * esize(prec) : 0;
  std::vector<uint8_t> packed(nelem * esize(prec) * (fused ? 2 : 1), 0);
  // one output channel per task: its weights (cin x taps floats, contiguous) are read once and stay in the core's cache, its
  // rows of the image(s) are whole 64-byte lines of its own (unit-major, as this loop ran before, every element was a cache
  // miss 160 KB from the last: loading the 95 M parameters of the 3d_affs net took 1.34 s of `bs predict`'s start, 0.71 s now;
  // tools/probe_load.py)
  host_parallel_for((size_t)p.cout, [&](size_t n_) {
    const int n = (int)n_;
    for (size_t u = 0; u < pc.entries.size(); ++u) {
      const PackEntry& e = pc.entries[u];
      if (e.dummy) continue;
      const size_t s = u / kUnitsPerStep, j = u % kUnitsPerStep;
      for (int kk = 0; kk < SUB; ++kk) {
        const int c = e.c0 + kk;
        if (c >= e.creal) break;
        float v;
        if (e.wsrc == 0) v = wm.data[((size_t)n * cin_m + (e.cin_base + c)) * ntap_m + e.tap];
        else v = wr.data[(size_t)n * cin_r + (e.cin_base + c)];
        const size_t idx = (s * KS * pc.Npad + n) * BKE + j * SUB + kk;
        if (prec == BSMI_PREC_F32) {
          ((float*)packed.data())[idx] = v;
        } else if (prec == BSMI_PREC_BF16) {
          ((uint16_t*)packed.data())[idx] = host_f32_to_bf16(v);
        } else {
          uint16_t hi, lo;
          split_bf16(v, hi, lo);
          uint16_t* w16 = (uint16_t*)packed.data();
          if (fused) {  // hi image, then the lo image of the same layout
            w16[idx] = hi;
            w16[idx + nelem] = lo;
          } else {
            const size_t blk = (size_t)pc.Npad * BKE;
            w16[idx] = hi;
            w16[idx + blk] = hi;
            w16[idx + 2 * blk] = lo;
          }
        }
      }
    }
  });
  BSMI_HIP(hipMalloc(&pc.w, packed.size()));
  BSMI_HIP(hipMemcpy(pc.w, packed.data(), packed.size(), hipMemcpyHostToDevice));
  BSMI_HIP(hipMalloc((void**)&pc.bias, bias.size() * sizeof(float)));
  BSMI_HIP(hipMemcpy(pc.bias, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice));
  pc.ready = true;
  return BSMI_OK;
}

int pack_wino(bsmi_unet* h, PassSite& p, int ci) {
  PackedWino& pw = p.wino[ci];
  release(pw);
  pw.fused_only = wino_narrow_last(h, p, ci);
  if (!wino_eligible(p, ci) && !pw.fused_only) return BSMI_OK;
  const HostWeight& wm = h->weights[p.prefix + ".conv_pass." + std::to_string(2 * ci) + ".weight"];
  const HostWeight& wr = h->weights[p.prefix + ".residual.0.weight"];
  const int cin_m = (int)wm.shape[1];
  // channels of V: every source tensor keeps its own padding to kChanPad
  pw.cin_of_v.clear();
  if (ci == 0) {
    int base = 0;
    for (int s = 0; s < p.nslots; ++s) {
      for (int c = 0; c < round_up(p.cin[s], kChanPad); ++c) pw.cin_of_v.push_back(c < p.cin[s] ? base + c : -1);
      base += p.cin[s];
    }
  } else {
    for (int c = 0; c < round_up(p.cout, kChanPad); ++c) pw.cin_of_v.push_back(c < p.cout ? c : -1);
  }
  pw.Cv = (int)pw.cin_of_v.size();
  pw.m = wino_tile_edge();
  pw.tile = choose_tile(p.cout);
  pw.Npad = round_up(p.cout, tile_bn(pw.tile));
  pw.wz = !pw.fused_only && pw.m == 4 && wino_z_site(h, p, ci);
  wino_units(pw.Cv, pw.units, pw.wz ? 1 : 3);
  {
    size_t image_elems = 0, batch_elems = 0;
    static const bool on_host = [] { const char* e = getenv("BSMI_WINO_PACK_HOST"); return e && e[0] == '1'; }();
    if (on_host) {   // (the host form of the transform: kept as the cross-check of the device one, tests/test_fullsize_gpu.py)
      std::vector<uint16_t> packed;
      wino_pack_weights(wm.data.data(), p.cout, cin_m, pw.cin_of_v, pw.Npad, pw.units, packed, image_elems, batch_elems, pw.m, pw.wz);
      BSMI_HIP(hipMalloc(&pw.w, packed.size() * 2));
      BSMI_HIP(hipMemcpy(pw.w, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
    } else {
      const int rc = wino_pack_weights_dev(wm.data.data(), p.cout, cin_m, pw.cin_of_v, pw.Npad, pw.units, pw.m, &pw.w, image_elems, batch_elems, pw.wz);
      if (rc) return rc;
    }
    pw.lo_image_bytes = image_elems * 2;
    pw.batch_bytes = batch_elems * 2;
  }
  // the cropped 1x1x1 residual branch of the last stage: its K-steps alone
  pw.res_entries.clear();
  if (ci == p.nconv - 1) {
    std::vector<PackEntry> all;
    build_entries(p, ci, BSMI_PREC_BF16X3, all);
    for (size_t u = 0; u + 1 < all.size(); u += kUnitsPerStep) {
      bool res = false;
      for (int j = 0; j < kUnitsPerStep; ++j) res |= !all[u + j].dummy && all[u + j].wsrc == 1;
      if (res)
        for (int j = 0; j < kUnitsPerStep; ++j) pw.res_entries.push_back(all[u + j]);
    }
    if ((pw.res_entries.size() / kUnitsPerStep) % 2)
      for (int j = 0; j < kUnitsPerStep; ++j) pw.res_entries.push_back(PackEntry{0, 0, 0, 0, 0, 0, 0, 0, 0, true, 0});
    const int64_t cin_r = wr.shape[1];
    auto pack_res = [&](const std::vector<PackEntry>& ents, void** w_out, size_t* lo_out) -> int {
      const size_t nsteps = ents.size() / kUnitsPerStep;
      const size_t nelem = (nsteps * (size_t)pw.Npad + kWeightRowSlack) * 32;
      std::vector<uint16_t> packed(2 * nelem, 0);
      for (size_t u = 0; u < ents.size(); ++u) {
        const PackEntry& e = ents[u];
        if (e.dummy) continue;
        const size_t s = u / kUnitsPerStep, j = u % kUnitsPerStep;
        for (int n = 0; n < p.cout; ++n)
          for (int kk = 0; kk < 16; ++kk) {
            const int c = e.c0 + kk;
            if (c >= e.creal) break;
            const float v = wr.data[(size_t)n * cin_r + (e.cin_base + c)];
            const size_t idx = (s * pw.Npad + n) * 32 + j * 16 + kk;
            split_bf16(v, packed[idx], packed[nelem + idx]);
          }
      }
      *lo_out = nelem * 2;
      BSMI_HIP(hipMalloc(w_out, packed.size() * 2));
      BSMI_HIP(hipMemcpy(*w_out, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
      return BSMI_OK;
    };
    int rc = pack_res(pw.res_entries, &pw.res_w, &pw.res_lo_image_bytes);
    if (rc) return rc;
    for (int part = 0; part < 2; ++part) pw.res_part[part].clear();
    if (p.nslots == 2) {  // the branch cut by source: the skip connection, the upsampled map (the last slot of the launch)
      const int up_slot = (ci == 0 ? 0 : 1) + 1;
      for (size_t u = 0; u + 1 < pw.res_entries.size(); u += kUnitsPerStep) {
        int slot = -1;
        for (int j = 0; j < kUnitsPerStep; ++j)
          if (!pw.res_entries[u + j].dummy) slot = pw.res_entries[u + j].slot;
        if (slot < 0) continue;  // the padding K-step of the whole list
        for (int j = 0; j < kUnitsPerStep; ++j) pw.res_part[slot == up_slot ? 1 : 0].push_back(pw.res_entries[u + j]);
      }
      for (int part = 0; part < 2; ++part) {
        if ((pw.res_part[part].size() / kUnitsPerStep) % 2)
          for (int j = 0; j < kUnitsPerStep; ++j) pw.res_part[part].push_back(PackEntry{0, 0, 0, 0, 0, 0, 0, 0, 0, true, 0});
        if ((rc = pack_res(pw.res_part[part], &pw.res_part_w[part], &pw.res_part_lo[part]))) return rc;
      }
    }
  }
  if (below_up_site(h, p, ci) && pw.m == 4) {
    // the skip connection alone in F(4x4) form: V holds its channels only
    pw.skip_cin_of_v.assign(pw.cin_of_v.begin(), pw.cin_of_v.begin() + round_up(p.cin[0], kChanPad));
    pw.skip_Cv = (int)pw.skip_cin_of_v.size();
    wino_units(pw.skip_Cv, pw.skip_units);
    size_t image_elems = 0, batch_elems = 0;
    int rc = wino_pack_weights_dev(wm.data.data(), p.cout, cin_m, pw.skip_cin_of_v, pw.Npad, pw.skip_units, pw.m, &pw.skip_w, image_elems, batch_elems);
    if (rc) return rc;
    pw.skip_lo_image_bytes = image_elems * 2;
    pw.skip_batch_bytes = batch_elems * 2;
    // the upsampled source as nine (3,1,1) convolutions of the low-resolution tensor: K = its channels x kz (wino_units'
    // order: 32-channel chunks, the three z taps inside a chunk), columns tap-major
    const int cpad_low = round_up(p.cin[1], kChanPad), cpad_out = round_up(p.cout, kChanPad);
    wino_units(cpad_low, pw.below_units);
    pw.below_dense = p.cout <= 64;   // narrow stage: the nine taps side by side in one wide GEMM (9 Cpad columns on the 320-column tile)
    pw.below_tile = pw.below_dense ? TILE_256x320 : pw.tile;
    pw.below_Npad = pw.below_dense ? round_up(9 * cpad_out, tile_bn(pw.below_tile)) : pw.Npad;
    const size_t nsteps = pw.below_units.size() / kUnitsPerStep;
    const size_t tap_elems = nsteps * (size_t)pw.below_Npad * 32;
    const size_t nelem = (pw.below_dense ? 1 : 9) * tap_elems + (size_t)kWeightRowSlack * 32;
    std::vector<uint16_t> packed(2 * nelem, 0);
    const bool dense = pw.below_dense;
    const int cin1 = p.cin[1], cbase = p.cin[0];
    host_parallel_for((size_t)p.cout, [&](size_t n_) {   // one output channel per task (pack_conv)
      const int n = (int)n_;
      for (size_t u = 0; u < pw.below_units.size(); ++u) {
        const WinoUnit& un = pw.below_units[u];
        if (un.dummy) continue;
        const size_t s = u / kUnitsPerStep, j = u % kUnitsPerStep;
        for (int kk = 0; kk < 16; ++kk) {
          const int c = un.vc0 + kk;
          if (c >= cin1) break;
          const float* g = wm.data.data() + (((size_t)n * cin_m + (cbase + c)) * 3 + un.kz) * 9;  // [ky][kx]
          for (int tap = 0; tap < 9; ++tap) {
            const size_t idx = dense ? (s * pw.below_Npad + (size_t)tap * cpad_out + n) * 32 + j * 16 + kk
                                     : (size_t)tap * tap_elems + (s * pw.below_Npad + n) * 32 + j * 16 + kk;
            split_bf16(g[tap], packed[idx], packed[nelem + idx]);
          }
        }
      }
    });
    pw.below_lo_image_bytes = nelem * 2;
    pw.below_batch_bytes = dense ? 0 : tap_elems * 2;
    BSMI_HIP(hipMalloc(&pw.below_w, packed.size() * 2));
    BSMI_HIP(hipMemcpy(pw.below_w, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
    pw.below_ready = true;
  }
  pw.ready = true;
  return BSMI_OK;
}

// unit list of the halo-resident form: per source slot, 16-channel chunk and z tap a phase; its in-plane taps two per K-step
static void build_entries_h16(const PassSite& p, int ci, std::vector<PackEntry>& out, std::vector<H16PhaseHost>& phases) {
  const bool last = ci == p.nconv - 1;
  const int* k = p.k[ci];
  const PackEntry dummy{0, 0, 0, 0, 0, 0, 0, 0, 0, true, 0};
  auto add_taps = [&](int slot, int cin_base, int creal) {
    const int cpad = round_up(creal, kChanPad);
    // z tap outermost: two consecutive 16-channel chunks of a voxel share a 128-byte line, so every other phase finds its
    // rows in L2
    for (int z = 0; z < k[0]; ++z)
      for (int c0 = 0; c0 < cpad; c0 += 16) {
        H16PhaseHost ph{slot, c0, z, 0, (int)(out.size() / kUnitsPerStep), 0};
        const int ntap = k[1] * k[2];
        for (int i = 0; i < ntap; i += 2) {
          for (int j = 0; j < 2; ++j) {
            if (i + j < ntap) {
              const int y = (i + j) / k[2], x = (i + j) % k[2];
              out.push_back(PackEntry{slot, z, y, x, c0, 0, (z * k[1] + y) * k[2] + x, cin_base, creal, false, (int)phases.size()});
            } else {
              out.push_back(dummy);
            }
          }
          ++ph.nsteps;
        }
        phases.push_back(ph);
      }
  };
  if (ci == 0) {
    int base = 0;
    for (int s = 0; s < p.nslots; ++s) {
      add_taps(s, base, p.cin[s]);
      base += p.cin[s];
    }
  } else {
    add_taps(0, 0, p.cout);
  }
  if (last) {
    int crop[3] = {0, 0, 0};
    for (int i = 0; i < p.nconv; ++i)
      for (int d = 0; d < 3; ++d) crop[d] += p.k[i][d] - 1;
    const int first_slot = ci == 0 ? 0 : 1;
    int base = 0;
    for (int s = 0; s < p.nslots; ++s) {
      const int cpad = round_up(p.cin[s], kChanPad);
      for (int c0 = 0; c0 < cpad; c0 += 16) {
        phases.push_back(H16PhaseHost{first_slot + s, c0, crop[0] / 2, 1, (int)(out.size() / kUnitsPerStep), 1});
        out.push_back(PackEntry{first_slot + s, crop[0] / 2, crop[1] / 2, crop[2] / 2, c0, 1, 0, base, p.cin[s], false, (int)phases.size() - 1});
        out.push_back(dummy);
      }
      base += p.cin[s];
    }
  }
}

int pack_h16(bsmi_unet* h, PassSite& p, int ci) {
  PackedH16& ph = p.h16[ci];
  release(ph);
  if (h16_mode() == 0 || p.cout > 64) return BSMI_OK;
  ph.entries.clear();
  ph.phases.clear();
  build_entries_h16(p, ci, ph.entries, ph.phases);
  ph.Npad = p.cout <= 16 ? 16 : 64;
  const HostWeight& wm = h->weights[p.prefix + ".conv_pass." + std::to_string(2 * ci) + ".weight"];
  const HostWeight& wr = h->weights[p.prefix + ".residual.0.weight"];
  const int64_t cin_m = wm.shape[1], ntap_m = wm.shape[2] * wm.shape[3] * wm.shape[4], cin_r = wr.shape[1];
  const size_t nsteps = ph.entries.size() / kUnitsPerStep;
  const size_t nelem = (nsteps * (size_t)ph.Npad + kWeightRowSlack) * 32;
  std::vector<uint16_t> packed(2 * nelem, 0);
  host_parallel_for((size_t)p.cout, [&](size_t n_) {   // one output channel per task (pack_conv)
    const int n = (int)n_;
    for (size_t u = 0; u < ph.entries.size(); ++u) {
      const PackEntry& e = ph.entries[u];
      if (e.dummy) continue;
      const size_t s = u / kUnitsPerStep, j = u % kUnitsPerStep;
      for (int kk = 0; kk < 16; ++kk) {
        const int c = e.c0 + kk;
        if (c >= e.creal) break;
        const float v = e.wsrc == 0 ? wm.data[((size_t)n * cin_m + (e.cin_base + c)) * ntap_m + e.tap] : wr.data[(size_t)n * cin_r + (e.cin_base + c)];
        const size_t idx = (s * ph.Npad + n) * 32 + j * 16 + kk;
        split_bf16(v, packed[idx], packed[nelem + idx]);
      }
    }
  });
  ph.lo_image_bytes = nelem * 2;
  BSMI_HIP(hipMalloc(&ph.w, packed.size() * 2));
  BSMI_HIP(hipMemcpy(ph.w, packed.data(), packed.size() * 2, hipMemcpyHostToDevice));
  ph.ready = true;
  return BSMI_OK;
}

}  // namespace bsmi

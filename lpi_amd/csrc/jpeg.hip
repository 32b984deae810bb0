// JPEG files -> packed HWC RGB uint8 pixels on the GPU (pixel_format='jpeg', lpi_amd/imageops.py), byte for byte what Pillow 12 (libjpeg-turbo,
// default settings) gives for np.asarray(Image.open(f).convert("RGB")): baseline files, with LPI_JPEG_PROGRESSIVE progressive files whose scan
// script is complete, with LPI_JPEG_LAYOUTS baseline files of more layouts (the first component 1x2, 4x1 or 1x4 over the others; RGB; four
// components, CMYK or YCCK).  tests/jpeg_restate.py, tests/jpeg_progressive.py and tests/jpeg_layouts.py restate every step in numpy / plain Python.
//
// The host parses the headers (parse_headers: the one place that decides the envelope; frame_in_envelope is the frame's share of it, the same for
// a baseline file and a progressive one) and lays the workspace out in one walk over the files (plan: one JDesc per image, its geometry from Geom,
// the entropy-coded bytes of every scan an EntRange that place_range fills), then copies the descriptors into the workspace; four launches do the rest
// for baseline files:
//   unstuff_kernel   one workgroup per image: the entropy-coded bytes without the 0xFF00 stuffing, split at the RSTn markers, up to the first other
//                    marker (rounds of 4096 bytes, a block-wide scan per round).  Out: the unstuffed bytes and the end of every restart interval.
//   huff_kernel      one workgroup per image: Huffman decoding.  Every restart interval (segment) is cut into k chunks.  A chunk's decoder state at
//                    a symbol boundary is (bit position, next coefficient index, block within the MCU).  The first chunk of a segment starts from the
//                    exact state; the others start speculatively at their first bit and run to their end.  Then each chunk re-decodes from its
//                    predecessor's exit state, until no exit state changes (self-synchronising decoding, Weissenberger & Schmidt): at most k
//                    rounds.  Block counts and DC sums per chunk give each chunk its first block and its DC predictors; a final pass writes the
//                    quantised coefficients.  A segment whose chunks do not add up to its MCUs, an invalid code, a coefficient index past 63, or
//                    a read past the segment's end sets the image's status: the caller then decodes that file on the host.
//   idct_kernel      one thread per 8x8 block: jidctint.c's islow IDCT with its range limit -> the component's sample plane.
//   color_kernel     one thread per output pixel: jdsample.c's fancy upsampling of the planes behind the first (2x1, 2x2; plain replication for
//                    planes at most 2 samples wide; 1x2 at every width; replication for 4x1 and 1x4), jdcolor.c's YCbCr -> RGB tables;
//                    grayscale replicated into R, G, B; RGB planes as they are; CMYK / YCCK through Pillow's inversion and convert("RGB").
// A file of four components is decoded by huff_kernel<4> (one more launch, only for a batch that has one); its fourth component's tables are a JExt.
//
// A progressive file (JDesc.k = 0: unstuff_kernel only clears its status, huff_kernel passes it over) has one PScan per scan, with the Huffman tables
// and the restart interval in force at its SOS; between huff_kernel and idct_kernel its coefficients are built up scan by scan (jdphuff.c):
//   punstuff_kernel  one workgroup per scan: unstuff_kernel's work (unstuff_range) on the scan's own EntRange.
//   pscan_kernel     one launch per ROUND of scans; one wave per scan.  The host puts a scan into round 1 + the latest round of an earlier scan that
//                    touched one of its (component, coefficient) pairs, so scans over the same coefficients run in file order and the others side by
//                    side (Pillow's 10 scans: 5 + 4 + 1).  A lane decodes one restart interval from its start: DC first / DC refinement / AC first
//                    (EOB runs) / AC refinement (correction bits, which depend on the coefficients of the earlier scans); a scan without restart
//                    markers is one lane's.  A one-component scan walks the component's own block grid, not the MCU-padded one.  A scan writes only
//                    the coefficients of its own band, one int16 at a time: the scans of a round share blocks.
// huff_kernel and pscan_kernel build their decoding tables with lut_codes / lut_entry and read codes with huff_symbol.
//
// Bounds: every loop runs over counts the host validated (rounds over the entropy bytes, symbols at most one per bit of a chunk, sync rounds at
// most k + 1; a progressive scan's MCUs, the coefficients of its band, at most LPI_JPEG_MAX_SCANS rounds); block indices come from those counts and
// coefficient indices stay inside [Ss, Se] whatever the bits say; the bit reader reads only its own image's (scan's) unstuffed bytes and returns
// zeros past its segment's end.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"

namespace {

constexpr int NT = 256;             // threads of the per-image workgroups of unstuff_kernel
constexpr int HT = 1024;            // threads of huff_kernel's per-image workgroups: up to HT chunks per image
constexpr int ROUND = NT * 16;      // entropy bytes per round of unstuff_kernel
constexpr int MIN_CHUNK = 64;       // bytes: shortest chunk the speculative decoder splits a segment into
constexpr int LUT_BITS = 9;

enum { ST_EOD = 1, ST_CODE = 2, ST_INDEX = 4, ST_COUNT = 8, ST_RST = 16 };

struct HuffSpec {
    uint8_t bits[16];
    uint8_t vals[256];
};

// The entropy-coded bytes of one scan (a baseline file's only one, or one of a progressive file's) and where they go.  Offsets: src_* into the
// caller's device bytes, ws_* into the workspace.
struct EntRange {
    long src_lo, src_hi;            // the scan's entropy-coded bytes
    long ws_unst, unst_cap;         // unstuffed bytes (capacity: src_hi - src_lo + 16)
    long ws_seg;                    // int32 end (unstuffed byte) of every segment
    int nseg, ri;                   // segments; restart interval in scan MCUs (a scan without restart markers: all of them)
};

// What libjpeg's output planes are, and so what color_kernel does with them (jdapimin.c default_decompress_parms, then Pillow's convert("RGB"))
enum { CT_GRAY = 0, CT_YCC = 1, CT_RGB = 2, CT_CMYK = 3, CT_YCCK = 4 };

// One image (device copy in the workspace's head).  out: offset into the caller's output, ws_*: into the workspace.  The workspace holds B of them
// in front of everything else, so sizeof(JDesc) is part of the workspace size of every batch: it stays at the 2320 bytes it had before
// LPI_JPEG_LAYOUTS (the fourth component's tables are a JExt behind the PScan table, which only a batch with such a file has).
struct JDesc {
    EntRange ent;                   // a baseline file's scan
    long out;                       // first byte of the h x w x 3 output
    long ws_coef[4];                // int16 [blocks][64] of each frame component
    long ws_plane[4];               // uint8 sample plane of each frame component
    long ws_ext;                    // a four-component file's JExt
    int w, h, nc, mcux, mcuy, bpm;
    int bw[4], bh[4];               // block grid of each frame component
    int scomp[4];                   // frame component of scan component s
    int hs, vs;                     // sampling of the first component over the others (which are 1x1); 1,1 for grayscale
    int dw, dh;                     // downsampled size of the other components
    int k;                          // chunks per segment
    int ct;                         // CT_*
    uint8_t blk_comp[10];           // scan component of block b of an MCU
    uint8_t blk_dx[10], blk_dy[10]; // its position inside the MCU's share of that component
    uint8_t spare[50];              // what the byte-sized block tables freed and the fourth component did not take: keeps the size (above)
    uint16_t qt[3][64];             // dequantisation table of each of the first three frame components, natural order
    HuffSpec dc[3], ac[3];          // tables of each of the first three scan components
};
static_assert(sizeof(JDesc) == 2320, "the workspace of a batch of three-component files must not change");

// The fourth component's tables of a four-component file (CMYK, YCCK).
struct JExt {
    uint16_t qt[64];
    HuffSpec dc, ac;
};

// One scan of a progressive file (device copies behind the sample planes in the workspace, sorted by launch round).
struct PScan {
    EntRange ent;
    long nmcu;                      // scan MCUs: the frame's MCUs (interleaved), or the blocks of the component's own grid
    int img;                        // its image's JDesc
    int ns, comp[3];                // frame components
    int ss, se, ah, al;
    int gw;                         // one-component scan: blocks per row of the component's own grid
    HuffSpec tab[3];                // first DC scan: the DC table of each scan component; AC scan: tab[0]
};

// Natural index of the coefficient at zigzag index z: the one list, read by the host parser and (as a constant the compiler emits for the device
// too) by the kernels.
constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// its inverse: v[n] = zigzag index of the coefficient at natural index n (compile-time indices only)
struct Unzigzag {
    int v[64];
    constexpr Unzigzag() : v() {
        for (int z = 0; z < 64; ++z) v[kZigzag[z]] = z;
    }
};
constexpr Unzigzag kUnzigzag;

// ------------------------------------------------------------------------------------------------------------------------------ host parser
// One scan of a progressive file: its entropy-coded bytes [ent, end) of the file, its header, the restart interval and the Huffman tables in force
// at its SOS (tab[i]: the DC table of scan component i for a first DC scan, tab[0]: the AC table of an AC scan), and the launch round it runs in.
struct ScanHd {
    long ent = 0, end = 0;
    int ns = 0, sc[3] = {}, ss = 0, se = 0, ah = 0, al = 0, ri = 0, level = 0;
    HuffSpec tab[3] = {};
};

struct Header {
    int w = 0, h = 0, nc = 0, prec = 0;
    int cid[4] = {}, ch[4] = {}, cv[4] = {}, ctq[4] = {};
    int ns = 0, sc[4] = {}, std_[4] = {}, sta[4] = {};
    int ri = 0;
    bool jfif = false, adobe = false, sof = false;
    int adobe_tf = 0;       // the Adobe APP14's transform byte
    bool qdef[4] = {}, hdef[2][4] = {};
    uint16_t qt[4][64] = {};
    HuffSpec hs[2][4] = {};
    long ent = 0;
    bool gpu = false;       // inside the envelope
    bool prog = false;      // SOF2, parsed with LPI_JPEG_PROGRESSIVE
    int lvl[3][64] = {};    // the launch round of the last scan that touched each coefficient of each component
    std::vector<ScanHd> scans;       // of a progressive file inside the envelope, in file order
};

inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

bool huff_ok(const HuffSpec& t, int count, bool dc) {
    long code = 0;
    for (int l = 0; l < 16; ++l) {
        code += t.bits[l];
        if (code >= (1L << (l + 1))) return false;     // jpeg_make_d_derived_tbl: the all-ones code is not a code
        code <<= 1;
    }
    if (dc)
        for (int i = 0; i < count; ++i)
            if (t.vals[i] > 15) return false;
    return true;
}

// What libjpeg takes the frame's components for (default_decompress_parms).  Three: a JFIF APP0 says YCbCr; else an Adobe APP14 says RGB with
// transform 0 and YCbCr with any other value; else the ids 'R','G','B' say RGB and any others YCbCr.  Four: an Adobe APP14 with a transform other
// than 0 says YCCK, anything else CMYK.
int color_transform(const Header& hd) {
    if (hd.nc == 1) return CT_GRAY;
    if (hd.nc == 4) return hd.adobe && hd.adobe_tf != 0 ? CT_YCCK : CT_CMYK;
    if (hd.jfif) return CT_YCC;
    if (hd.adobe) return hd.adobe_tf == 0 ? CT_RGB : CT_YCC;
    return hd.cid[0] == 'R' && hd.cid[1] == 'G' && hd.cid[2] == 'B' ? CT_RGB : CT_YCC;
}

// The frame's share of the envelope, whatever its scans are: 8-bit, a height in the header, a size the decoder's workspace and its int bit positions
// take, and grayscale or the three components libjpeg takes for YCbCr with luma sampled 1x1, 2x1 or 2x2 over 1x1 chroma.  layouts
// (LPI_JPEG_LAYOUTS, baseline files only): three components of any marking (color_transform) or four, the first sampled 1x1, 2x1, 2x2, 1x2, 4x1 or
// 1x4 over the others at 1x1.
bool frame_in_envelope(const Header& hd, bool layouts) {
    if (hd.prec != 8 || hd.h <= 0 || (long)hd.w * hd.h > LPI_JPEG_MAX_PIXELS) return false;
    if (hd.nc == 1) return true;
    if (hd.nc != 3 && !(layouts && hd.nc == 4)) return false;
    if (!layouts && !hd.jfif && (hd.adobe || (hd.cid[0] == 'R' && hd.cid[1] == 'G' && hd.cid[2] == 'B'))) return false;
    for (int c = 1; c < hd.nc; ++c)
        if (hd.ch[c] != 1 || hd.cv[c] != 1) return false;
    const int H = hd.ch[0], V = hd.cv[0];
    if ((H == 1 && V == 1) || (H == 2 && V == 1) || (H == 2 && V == 2)) return true;
    return layouts && ((H == 1 && V == 2) || (H == 4 && V == 1) || (H == 1 && V == 4));
}

// One SOS of a SOF2 file against the progressive envelope; appends it to hd.scans.  false: the file is the host's.
bool progressive_scan(Header& hd, const uint8_t* s, long ent, long end, int (*al_cur)[64]) {
    if (hd.scans.empty()) {
        if (!frame_in_envelope(hd, false)) return false;        // the new layouts are baseline files only: pscan_kernel holds three tables
        hd.ent = ent;
    }
    if ((int)hd.scans.size() >= LPI_JPEG_MAX_SCANS || hd.ns > 3) return false;
    ScanHd sc;
    sc.ent = ent;
    sc.end = end;
    sc.ns = hd.ns;
    sc.ss = s[1 + 2 * hd.ns];
    sc.se = s[2 + 2 * hd.ns];
    sc.ah = s[3 + 2 * hd.ns] >> 4;
    sc.al = s[3 + 2 * hd.ns] & 15;
    sc.ri = hd.ri;
    for (int i = 0; i < hd.ns; ++i) {
        sc.sc[i] = hd.sc[i];
        if (i > 0 && hd.sc[i] <= hd.sc[i - 1]) return false;           // an interleaved scan lists its components in the frame's order
    }
    if (sc.al > 13 || sc.ss > sc.se || sc.se > 63) return false;
    if (sc.ss == 0 ? sc.se != 0 : sc.ns != 1) return false;            // DC scans hold DC only; AC scans hold one component
    if (sc.ah != 0 && sc.al != sc.ah - 1) return false;
    int level = 0;
    for (int i = 0; i < sc.ns; ++i) {
        const int c = sc.sc[i];
        if (sc.ss > 0 && al_cur[c][0] < 0) return false;               // AC before the component's first DC scan
        for (int k = sc.ss; k <= sc.se; ++k) {
            if (sc.ah == 0 ? al_cur[c][k] != -1 : al_cur[c][k] != sc.ah) return false;
            al_cur[c][k] = sc.al;
            level = std::max(level, hd.lvl[c][k]);
        }
        if (sc.ss == 0 && sc.ah == 0) {
            if (!hd.hdef[0][hd.std_[i]]) return false;
            sc.tab[i] = hd.hs[0][hd.std_[i]];
        } else if (sc.ss > 0) {
            if (!hd.hdef[1][hd.sta[i]]) return false;
            sc.tab[0] = hd.hs[1][hd.sta[i]];
        }
    }
    // scans over the same (component, coefficient) run in file order: round = 1 + the latest round of an earlier scan that touched one of them
    sc.level = level + 1;
    for (int i = 0; i < sc.ns; ++i)
        for (int k = sc.ss; k <= sc.se; ++k) hd.lvl[sc.sc[i]][k] = sc.level;
    hd.scans.push_back(sc);
    return true;
}

// 0: parsed (hd.gpu says whether the GPU decodes it); LPI_EINVAL: a structural error in the headers.  A file without SOI is parsed as "host".
// flags & LPI_JPEG_PROGRESSIVE: a SOF2 file is parsed to its end (every SOS, the DHT / DRI between the scans) and is inside the envelope when its
// scan script is complete and orderly (include/lpi_hip.h); hd.scans then holds its scans.  Without the flag a SOF2 file is the host's at its SOF.
// flags & LPI_JPEG_LAYOUTS: the wider frame rule of frame_in_envelope for SOF0 / SOF1 files.
int parse_headers(const uint8_t* d, long n, Header& hd, int flags = 0) {
    hd = Header();
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return 0;
    long p = 2;
    int al_cur[3][64];                      // progressive: the Al every coefficient of every component has been decoded to (-1: not yet)
    for (auto& c : al_cur)
        for (int& v : c) v = -1;
    for (int guard = 0; guard < (1 << 20); ++guard) {
        while (p + 1 < n && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
        if (hd.prog && !hd.scans.empty() && (p + 1 >= n || (d[p] == 0xFF && d[p + 1] == 0xD9))) {
            // EOI, or the end of the data (a truncated file: the decoder then meets the end of its last scan): the script must be complete
            bool ok = true;
            for (int c = 0; c < hd.nc; ++c)
                for (int k = 0; k < 64; ++k) ok = ok && al_cur[c][k] == 0;
            ok = ok && n - hd.ent <= LPI_JPEG_MAX_SCAN_BYTES;
            hd.gpu = ok;
            if (!ok) hd.scans.clear();
            return 0;
        }
        if (p + 4 > n || d[p] != 0xFF) return LPI_EINVAL;
        const int m = d[p + 1];
        if (m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7) || m == 0x01 || m == 0x00) return LPI_EINVAL;
        const long L = rd16(d + p + 2);
        if (L < 2 || p + 2 + L > n) return LPI_EINVAL;
        const uint8_t* s = d + p + 4;
        const long sl = L - 2;
        p += 2 + L;
        if (m == 0xC0 || m == 0xC1 || (m == 0xC2 && (flags & LPI_JPEG_PROGRESSIVE))) {
            if (hd.sof || sl < 6) return LPI_EINVAL;
            hd.prec = s[0];
            hd.h = rd16(s + 1);
            hd.w = rd16(s + 3);
            hd.nc = s[5];
            if (hd.nc < 1 || hd.nc > 4 || sl != 6 + 3 * hd.nc || hd.w == 0) return LPI_EINVAL;
            for (int i = 0; i < hd.nc; ++i) {
                hd.cid[i] = s[6 + 3 * i];
                hd.ch[i] = s[7 + 3 * i] >> 4;
                hd.cv[i] = s[7 + 3 * i] & 15;
                hd.ctq[i] = s[8 + 3 * i];
                if (hd.ch[i] < 1 || hd.ch[i] > 4 || hd.cv[i] < 1 || hd.cv[i] > 4 || hd.ctq[i] > 3) return LPI_EINVAL;
            }
            hd.sof = true;
            hd.prog = m == 0xC2;
        } else if ((m >= 0xC2 && m <= 0xCF) && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            if (hd.prog) return LPI_EINVAL;                     // a second frame header
            if (sl >= 6) {                                      // progressive, lossless, arithmetic-coded, hierarchical: the host decodes
                hd.h = rd16(s + 1);
                hd.w = rd16(s + 3);
                hd.nc = s[5];
            }
            return 0;
        } else if (m == 0xCC) {
            return 0;                                           // arithmetic conditioning tables
        } else if (m == 0xC4) {
            long q = 0;
            while (q < sl) {
                if (q + 17 > sl) return LPI_EINVAL;
                const int tc = s[q] >> 4, th = s[q] & 15;
                int cnt = 0;
                for (int l = 0; l < 16; ++l) cnt += s[q + 1 + l];
                if (tc > 1 || th > 3 || cnt > 256 || q + 17 + cnt > sl) return LPI_EINVAL;
                HuffSpec& t = hd.hs[tc][th];
                std::memset(&t, 0, sizeof(t));
                std::memcpy(t.bits, s + q + 1, 16);
                std::memcpy(t.vals, s + q + 17, (size_t)cnt);
                if (!huff_ok(t, cnt, tc == 0)) return LPI_EINVAL;
                hd.hdef[tc][th] = true;
                q += 17 + cnt;
            }
        } else if (m == 0xDB) {
            if (!hd.scans.empty()) { hd.scans.clear(); return 0; }          // quantisation tables between the scans: the host's
            long q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                const long size = 64L * (pq + 1);
                if (pq > 1 || tq > 3 || q + 1 + size > sl) return LPI_EINVAL;
                for (int i = 0; i < 64; ++i) hd.qt[tq][kZigzag[i]] = (uint16_t)(pq ? rd16(s + q + 1 + 2 * i) : s[q + 1 + i]);
                hd.qdef[tq] = true;
                q += 1 + size;
            }
        } else if (m == 0xDD) {
            if (sl != 2) return LPI_EINVAL;
            hd.ri = rd16(s);
        } else if (m == 0xE0) {
            if (sl >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) hd.jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
                hd.adobe = true;
                hd.adobe_tf = s[11];
            }
        } else if (m == 0xDA) {
            if (!hd.sof || sl < 1) return LPI_EINVAL;
            hd.ns = s[0];
            if (hd.ns < 1 || hd.ns > 4 || sl != 4 + 2 * hd.ns) return LPI_EINVAL;
            for (int i = 0; i < hd.ns; ++i) {
                int f = -1;
                for (int c = 0; c < hd.nc; ++c)
                    if (hd.cid[c] == s[1 + 2 * i]) f = c;
                if (f < 0) return LPI_EINVAL;
                for (int j = 0; j < i; ++j)
                    if (hd.sc[j] == f) return LPI_EINVAL;
                hd.sc[i] = f;
                hd.std_[i] = s[2 + 2 * i] >> 4;
                hd.sta[i] = s[2 + 2 * i] & 15;
                if (hd.std_[i] > 3 || hd.sta[i] > 3) return LPI_EINVAL;
                if (!hd.prog && (!hd.hdef[0][hd.std_[i]] || !hd.hdef[1][hd.sta[i]])) return LPI_EINVAL;
            }
            for (int c = 0; c < hd.nc; ++c)
                if (!hd.qdef[hd.ctq[c]]) return LPI_EINVAL;
            if (hd.prog) {
                // the scan's entropy-coded bytes: up to the next marker that is neither a stuffed 0xFF00 nor RSTn (as unstuff_range reads them)
                long q = p;
                while (q < n) {
                    const void* f = std::memchr(d + q, 0xFF, (size_t)(n - q));
                    if (!f) { q = n; break; }
                    q = static_cast<const uint8_t*>(f) - d;
                    if (q + 1 >= n) break;
                    const int nx = d[q + 1];
                    if (nx == 0x00 || (nx >= 0xD0 && nx <= 0xD7)) q += 2;
                    else if (nx == 0xFF) q += 1;
                    else break;
                }
                if (!progressive_scan(hd, s, p, q, al_cur)) { hd.scans.clear(); return 0; }
                p = q;
                continue;
            }
            hd.ent = p;
            const int ss = s[1 + 2 * hd.ns], se = s[2 + 2 * hd.ns], ahal = s[3 + 2 * hd.ns];
            bool ok = frame_in_envelope(hd, (flags & LPI_JPEG_LAYOUTS) != 0) && hd.ns == hd.nc && ss == 0 && se == 63 && ahal == 0;
            // libjpeg-turbo's get_sos looks a scan component up among the frame components whose slot in the SCAN's list is still empty: a
            // full scan in any order but the frame's ends in JERR_BAD_COMPONENT_ID, so such files are Pillow's (its exception)
            for (int i = 0; i < hd.ns; ++i) ok = ok && hd.sc[i] == i;
            hd.gpu = ok && n - hd.ent <= LPI_JPEG_MAX_SCAN_BYTES;          // as the frame's size: what the int bit positions take
            return 0;
        }
        // APPn, COM, DNL and anything else with a length: skipped
    }
    return LPI_EINVAL;
}

// ------------------------------------------------------------------------------------------------------------------------------ plan
inline long align256(long v) { return (v + 255) / 256 * 256; }

// A frame's geometry: the MCU's size in blocks (1 x 1 for grayscale, whatever its sampling factors say), the MCU grid, every component's share.
struct Geom {
    int hm, vm, mcux, mcuy;
    int H[4], V[4];
    explicit Geom(const Header& hd) {
        for (int c = 0; c < 4; ++c) {
            H[c] = hd.nc == 1 ? 1 : hd.ch[c];
            V[c] = hd.nc == 1 ? 1 : hd.cv[c];
        }
        hm = H[0];
        vm = V[0];
        mcux = (hd.w + 8 * hm - 1) / (8 * hm);
        mcuy = (hd.h + 8 * vm - 1) / (8 * vm);
    }
    long nmcu() const { return (long)mcux * mcuy; }
};

// Scan MCUs of one scan of a progressive file: the frame's MCUs for an interleaved scan; for a one-component scan the blocks of the component's own
// grid, ceil(cw / 8) x ceil(ch / 8) with cw = ceil(w * Hc / Hmax) (gw: its blocks per row), not the MCU-padded grid the coefficient arrays have.
inline long scan_mcus(const Header& hd, const Geom& g, const ScanHd& sc, int* gw) {
    if (sc.ns > 1) {
        *gw = 0;
        return g.nmcu();
    }
    const int c = sc.sc[0];
    const long cw = ((long)hd.w * g.H[c] + g.hm - 1) / g.hm, chh = ((long)hd.h * g.V[c] + g.vm - 1) / g.vm;
    *gw = (int)((cw + 7) / 8);
    return (long)*gw * ((chh + 7) / 8);
}

// A scan of nmcu scan MCUs with the entropy-coded bytes src[lo, hi): its unstuffed bytes and its segment table placed at `at`, which moves past
// them.  ri: the restart interval at its SOS; 0 makes the whole scan one interval.
EntRange place_range(long lo, long hi, long nmcu, int ri, long& at) {
    EntRange e;
    e.src_lo = lo;
    e.src_hi = hi;
    e.ri = ri ? ri : (int)std::min(nmcu, (long)0x7fffffff);
    e.nseg = (int)((nmcu + e.ri - 1) / e.ri);
    e.unst_cap = hi - lo + 16;
    e.ws_unst = at;
    at += align256(e.unst_cap);
    e.ws_seg = at;
    at += align256((long)e.nseg * 4);
    return e;
}

// What one decode call needs.  The workspace, every part rounded up to 256 bytes: the descriptors; every scan's unstuffed bytes and segment table,
// in file order and scan order; every image's coefficient arrays, [zero_lo, zero_hi), which the caller clears before huff_kernel; every image's
// sample planes; at ws_scans the PScan table (behind everything a batch of baseline files has: such a batch needs the same bytes with and without
// the flag), at ws_exts the JExt table.  scans: sorted by launch round, rounds[r] of them run in round r.
struct Plan {
    std::vector<JDesc> descs;
    std::vector<PScan> scans;
    std::vector<int> rounds;
    std::vector<JExt> exts;         // of the four-component files, at ws_exts behind the PScan table
    long bytes = 0, zero_lo = 0, zero_hi = 0, ws_scans = 0, ws_exts = 0;
};

// 0, or LPI_EINVAL (an argument, or a file with a structural error or outside the envelope of `flags`).  A progressive file gets a JDesc with
// k = 0, which the baseline kernels pass over, and one PScan per scan.
int plan(int flags, int B, const uint8_t* host, const long* offsets, Plan& pl) {
    if (B < 1 || B > 65535 || !host || !offsets || (flags & ~LPI_JPEG_FLAGS)) return LPI_EINVAL;
    pl.descs.assign(B, JDesc());
    std::vector<PScan> ps;              // in file order
    std::vector<int> level;
    Header hd;
    long at = align256((long)B * (long)sizeof(JDesc)), coef = 0, plane = 0;        // coef, plane: from the start of their regions
    for (int i = 0; i < B; ++i) {
        if (offsets[i] < 0 || offsets[i + 1] < offsets[i] + 4) return LPI_EINVAL;
        if (parse_headers(host + offsets[i], offsets[i + 1] - offsets[i], hd, flags) != 0 || !hd.gpu) return LPI_EINVAL;
        const Geom g(hd);
        JDesc& j = pl.descs[i];
        JExt ext = JExt();
        j.w = hd.w;
        j.h = hd.h;
        j.nc = hd.nc;
        j.ct = color_transform(hd);
        j.hs = g.hm;
        j.vs = g.vm;
        j.mcux = g.mcux;
        j.mcuy = g.mcuy;
        j.dw = (hd.w + g.hm - 1) / g.hm;
        j.dh = (hd.h + g.vm - 1) / g.vm;
        for (const ScanHd& sc : hd.scans) {             // a progressive file's
            PScan q = PScan();
            q.nmcu = scan_mcus(hd, g, sc, &q.gw);
            q.ent = place_range(offsets[i] + sc.ent, offsets[i] + sc.end, q.nmcu, sc.ri, at);
            q.img = i;
            q.ns = sc.ns;
            for (int c = 0; c < 3; ++c) q.comp[c] = sc.sc[c];
            q.ss = sc.ss;
            q.se = sc.se;
            q.ah = sc.ah;
            q.al = sc.al;
            std::memcpy(q.tab, sc.tab, sizeof(q.tab));
            ps.push_back(q);
            level.push_back(sc.level);
        }
        if (!hd.prog) {
            j.ent = place_range(offsets[i] + hd.ent, offsets[i + 1], g.nmcu(), hd.ri, at);
            for (int s = 0; s < hd.ns; ++s) {
                const int f = hd.sc[s];
                j.scomp[s] = f;
                (s < 3 ? j.dc[s] : ext.dc) = hd.hs[0][hd.std_[s]];
                (s < 3 ? j.ac[s] : ext.ac) = hd.hs[1][hd.sta[s]];
                for (int y = 0; y < g.V[f]; ++y)
                    for (int x = 0; x < g.H[f]; ++x) {
                        j.blk_comp[j.bpm] = (uint8_t)s;
                        j.blk_dx[j.bpm] = (uint8_t)x;
                        j.blk_dy[j.bpm] = (uint8_t)y;
                        ++j.bpm;
                    }
            }
            // chunks per segment: at least MIN_CHUNK bytes each on average, at most HT chunks per image (one per thread); 1 when segments are many
            const long by_len = (j.ent.src_hi - j.ent.src_lo) / ((long)j.ent.nseg * MIN_CHUNK);
            j.k = (int)std::max(1L, std::min(j.ent.nseg <= HT / 2 ? (long)(HT / j.ent.nseg) : 1L, by_len));
        }
        for (int c = 0; c < hd.nc; ++c) {
            j.bw[c] = g.mcux * g.H[c];
            j.bh[c] = g.mcuy * g.V[c];
            std::memcpy(c < 3 ? j.qt[c] : ext.qt, hd.qt[hd.ctq[c]], sizeof(ext.qt));
            j.ws_coef[c] = coef;
            coef += (long)j.bw[c] * j.bh[c] * 128;
            j.ws_plane[c] = plane;
            plane += (long)j.bw[c] * j.bh[c] * 64;
        }
        coef = align256(coef);
        plane = align256(plane);
        if (hd.nc == 4) {
            j.ws_ext = (long)pl.exts.size() * (long)sizeof(JExt);
            pl.exts.push_back(ext);
        }
    }
    pl.zero_lo = at;
    pl.zero_hi = pl.zero_lo + coef;
    pl.ws_scans = pl.zero_hi + plane;
    pl.ws_exts = pl.ws_scans + align256((long)ps.size() * (long)sizeof(PScan));
    pl.bytes = pl.ws_exts + align256((long)pl.exts.size() * (long)sizeof(JExt));
    for (JDesc& j : pl.descs) {
        j.ws_ext += pl.ws_exts;
        for (int c = 0; c < j.nc; ++c) {
            j.ws_coef[c] += pl.zero_lo;
            j.ws_plane[c] += pl.zero_hi;
        }
    }
    pl.rounds.assign(LPI_JPEG_MAX_SCANS + 1, 0);
    for (int r = 1; r <= LPI_JPEG_MAX_SCANS; ++r)
        for (size_t q = 0; q < ps.size(); ++q)
            if (level[q] == r) {
                pl.scans.push_back(ps[q]);
                ++pl.rounds[r];
            }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------ kernels
__device__ inline int block_excl_scan(int v, int* sh, int& total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {
        const int a = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += a;
        __syncthreads();
    }
    total = sh[NT - 1];
    const int r = sh[t] - v;
    __syncthreads();
    return r;
}

// One workgroup: the bytes of range r without the stuffing into its unstuffed bytes, the end of each of its restart intervals into its segment
// table.  Returns the status flags (valid in thread 0).  sh: NT ints of LDS, s_end: one long.
__device__ inline int unstuff_range(const EntRange& r, const uint8_t* __restrict__ src, uint8_t* __restrict__ ws, int* sh, long* s_end_p) {
    const long lo = r.src_lo, hi = r.src_hi;
    uint8_t* __restrict__ un = ws + r.ws_unst;
    int* __restrict__ seg = reinterpret_cast<int*>(ws + r.ws_seg);
    const int nseg = r.nseg;
    long& s_end = *s_end_p;
    const int t = threadIdx.x;
    long emitted = 0;
    int nrst = 0, flags = 0;
    if (t == 0) s_end = hi;
    __syncthreads();
    for (long base = lo; base < hi; base += ROUND) {
        const long i0 = base + 16L * t;
        // 1: the first marker other than RSTn in this round
        long my_end = hi;
        for (int q = 0; q < 16; ++q) {
            const long i = i0 + q;
            if (i >= hi) break;
            if (src[i] != 0xFF) continue;
            if (i + 1 >= hi) { my_end = i; break; }
            const int nx = src[i + 1];
            if (nx != 0x00 && nx != 0xFF && !(nx >= 0xD0 && nx <= 0xD7)) { my_end = i; break; }
        }
        if (my_end < hi) atomicMin((unsigned long long*)&s_end, (unsigned long long)my_end);
        __syncthreads();
        const long e = s_end;
        // 2: counts and offsets of the data bytes and RSTn markers before e
        int ne = 0, nr = 0;
        for (int q = 0; q < 16; ++q) {
            const long i = i0 + q;
            if (i >= e) break;
            const int b = src[i];
            const int prev = i > lo ? src[i - 1] : 0;
            if (b != 0xFF) ne += prev != 0xFF;
            else {
                const int nx = src[i + 1];           // i + 1 < e <= hi: a lone trailing 0xFF is an end
                ne += nx == 0x00;
                nr += nx >= 0xD0 && nx <= 0xD7;
            }
        }
        int tot_e = 0, tot_r = 0;
        const int oe = block_excl_scan(ne, sh, tot_e);
        const int orr = block_excl_scan(nr, sh, tot_r);
        // 3: write
        long w = emitted + oe;
        int r = nrst + orr;
        for (int q = 0; q < 16; ++q) {
            const long i = i0 + q;
            if (i >= e) break;
            const int b = src[i];
            const int prev = i > lo ? src[i - 1] : 0;
            if (b != 0xFF) {
                if (prev != 0xFF) un[w++] = (uint8_t)b;
            } else {
                const int nx = src[i + 1];
                if (nx == 0x00) un[w++] = 0xFF;
                else if (nx >= 0xD0 && nx <= 0xD7) {
                    if (nx != 0xD0 + (r & 7) || r >= nseg - 1) flags |= ST_RST;
                    else seg[r] = (int)w;
                    ++r;
                }
            }
        }
        emitted += tot_e;
        nrst += tot_r;
        if (e < base + ROUND) break;
    }
    if (t == 0) {
        if (nrst != nseg - 1) flags |= ST_RST;
        seg[nseg - 1] = (int)emitted;
        for (int q = 0; q < 16; ++q) un[emitted + q] = 0;      // the reader's tail: inside unst_cap (emitted <= entropy bytes)
    }
    __syncthreads();
    sh[t] = flags;
    __syncthreads();
    int f = 0;
    if (t == 0)
        for (int q = 0; q < NT; ++q) f |= sh[q];
    return f;
}

__global__ __launch_bounds__(NT) void unstuff_kernel(const JDesc* __restrict__ descs, const uint8_t* __restrict__ src, uint8_t* __restrict__ ws,
                                                     int* __restrict__ status) {
    __shared__ int sh[NT];
    __shared__ long s_end;
    const JDesc& d = descs[blockIdx.x];
    if (d.k == 0) {                                 // a progressive file: its scans are punstuff_kernel's, which adds to this status
        if (threadIdx.x == 0) status[blockIdx.x] = 0;
        return;
    }
    const int f = unstuff_range(d.ent, src, ws, sh, &s_end);
    if (threadIdx.x == 0) status[blockIdx.x] = f;
}

// grid: the scans of the batch's progressive files
__global__ __launch_bounds__(NT) void punstuff_kernel(const PScan* __restrict__ scans, const uint8_t* __restrict__ src, uint8_t* __restrict__ ws,
                                                      int* __restrict__ status) {
    __shared__ int sh[NT];
    __shared__ long s_end;
    const PScan& sc = scans[blockIdx.x];
    const int f = unstuff_range(sc.ent, src, ws, sh, &s_end);
    if (threadIdx.x == 0 && f) atomicOr(status + sc.img, f);
}

struct Lut {
    uint16_t lut[1 << LUT_BITS];    // (length << 8) | symbol of codes up to LUT_BITS long; 0: longer
    int maxcode[17];                // largest code of each length (-1: none)
    int valoff[17];                 // vals index = code + valoff[length]
    uint8_t vals[256];
};

struct DecState {
    int p, z, b;
};

// Bit reader over one segment's unstuffed bytes [0, E) (bits), zeros past E.
struct Reader {
    const uint8_t* un;
    long cap;          // bytes that may be read
    int E;
    int wbyte;
    uint64_t win;
    __device__ void fill(int p) {
        wbyte = (p >> 5) << 2;
        uint64_t v = 0;
        if ((long)wbyte + 8 <= cap) {
            const uint32_t a = *reinterpret_cast<const uint32_t*>(un + wbyte), c = *reinterpret_cast<const uint32_t*>(un + wbyte + 4);
            v = ((uint64_t)__builtin_bswap32(a) << 32) | __builtin_bswap32(c);
        }
        const long keep = (long)E - (long)wbyte * 8;
        if (keep <= 0) v = 0;
        else if (keep < 64) v &= ~0ull << (64 - keep);
        win = v;
    }
    __device__ uint32_t peek32(int p) {
        if (p - wbyte * 8 > 32 || p < wbyte * 8) fill(p);
        return (uint32_t)((win << (p - wbyte * 8)) >> 32);
    }
};

__device__ inline int extend(int v, int s) { return s && v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// The code at the head of w32: returns its length (0: not a code) and its symbol.
__device__ inline int huff_symbol(const Lut& L, uint32_t w32, int& sym) {
    const uint32_t w16 = w32 >> 16;
    const int e = L.lut[w16 >> (16 - LUT_BITS)];
    if (e) {
        sym = e & 255;
        return e >> 8;
    }
    for (int l = LUT_BITS + 1; l <= 16; ++l) {
        const int code = (int)(w16 >> (16 - l));
        if (code <= L.maxcode[l]) {
            sym = L.vals[(code + L.valoff[l]) & 255];
            return l;
        }
    }
    return 0;
}

// The decoding tables of one Huffman table: the code ranges per length, then the short-code lookup entry by entry.
__device__ inline void lut_codes(const HuffSpec& hs, Lut& L) {
    int code = 0, k = 0;
    L.maxcode[0] = -1;
    L.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = hs.bits[l - 1];
        L.valoff[l] = k - code;
        code += n;
        k += n;
        L.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
    for (int q = 0; q < 256; ++q) L.vals[q] = hs.vals[q];
}

__device__ inline uint16_t lut_entry(const Lut& L, int e) {
    for (int l = 1; l <= LUT_BITS; ++l) {
        const int code = e >> (LUT_BITS - l);
        if (code <= L.maxcode[l]) return (uint16_t)((l << 8) | L.vals[(code + L.valoff[l]) & 255]);
    }
    return 0;
}

// Where block b of an MCU goes: its scan component, and the position of its 8x8 block inside the MCU's share of that component (huff_kernel's LDS)
struct BlkInfo {
    int sc, dx, dy, H, V, bw;
    long coef;          // workspace byte offset of the component's coefficient blocks
};

// Decodes symbols from st until `want` blocks are complete or, for stop_bit >= 0, the first symbol boundary at or after stop_bit.  Returns the
// blocks completed; dcs: the DC differences summed per scan component.  ws != nullptr: writes the coefficients of blocks first + 0, 1, ...
// (blocks past `limit` are not written) with the DC predictors pred.  Invalid data: flags, and a deterministic way on (the state stays a function of
// the bits, which is all the synchronisation needs).
__device__ int decode_run(const BlkInfo* __restrict__ bi, int bpm, int mcux, const int* __restrict__ zz, const Lut* __restrict__ dl,
                          const Lut* __restrict__ al, Reader& rd, DecState& st, int stop_bit, int want, int* dcs, int* flags, uint8_t* ws, long first,
                          long limit, int* pred) {
    int nb = 0;
    int sc = bi[st.b].sc;
    auto locate = [&](long g) -> int16_t* {            // the coefficients of block g (the current block st.b), or nullptr
        if (!ws || g >= limit) return nullptr;
        const BlkInfo& q = bi[st.b];
        const long m = g / bpm;
        const long bx = (m % mcux) * q.H + q.dx, by = (m / mcux) * q.V + q.dy;
        return reinterpret_cast<int16_t*>(ws + q.coef) + (by * q.bw + bx) * 64;
    };
    int16_t* bp = st.z > 0 ? locate(first) : nullptr;    // a block the previous chunk began
    const int maxsym = (stop_bit >= 0 ? stop_bit - st.p : rd.E - st.p) + 64;     // every symbol takes at least one bit
    for (int it = 0; it < maxsym; ++it) {
        if (nb >= want || (stop_bit >= 0 && st.p >= stop_bit)) break;
        if (stop_bit < 0 && st.p > rd.E) break;
        const uint32_t w32 = rd.peek32(st.p);
        const Lut& L = st.z == 0 ? dl[sc] : al[sc];
        int sym = 0;
        const int len = huff_symbol(L, w32, sym);
        if (!len) {                                  // invalid code
            *flags |= ST_CODE;
            st.p += 1;
            continue;
        }
        const int s = sym & 15;
        const int v = s ? extend((int)((w32 << len) >> (32 - s)), s) : 0;
        st.p += len + s;
        bool done = false;
        if (st.z == 0) {
            dcs[sc] += v;
            bp = locate(first + nb);
            if (bp) {
                pred[sc] += v;
                bp[0] = (int16_t)pred[sc];
            }
            st.z = 1;
        } else {
            const int r = sym >> 4;
            if (s) {
                st.z += r;
                if (st.z > 63) {
                    *flags |= ST_INDEX;
                    done = true;
                } else {
                    if (bp) bp[zz[st.z]] = (int16_t)v;
                    ++st.z;
                    done = st.z > 63;
                }
            } else if (r == 15) {
                st.z += 16;
                done = st.z > 63;
            } else {
                done = true;
            }
        }
        if (done) {
            st.z = 0;
            st.b = st.b + 1 == bpm ? 0 : st.b + 1;
            sc = bi[st.b].sc;
            ++nb;
        }
    }
    return nb;
}

// NS: the scan components the workgroup has tables and DC sums for.  huff_kernel<3> decodes the files of one or three components and passes over
// those of four, huff_kernel<4> (launched only for a batch that has one) the reverse: the fourth component's tables and sums cost LDS that the
// other files need not pay for.
template <int NS>
__global__ __launch_bounds__(HT) void huff_kernel(const JDesc* __restrict__ descs, uint8_t* __restrict__ ws, int* __restrict__ status) {
    __shared__ Lut luts[2 * NS];
    __shared__ BlkInfo s_bi[10];
    __shared__ int s_zz[64];
    __shared__ int s_ep[HT], s_ez[HT], s_eb[HT];        // exit state of each chunk
    __shared__ int s_np[HT], s_nz[HT], s_nb[HT];        // entry state of each chunk
    __shared__ int s_cnt[HT], s_dc[HT][NS];              // blocks and DC sums from entry to exit; after the scan: those of the chunks before
    __shared__ int s_need[HT];
    __shared__ int s_any, s_flags;
    const JDesc& d = descs[blockIdx.x];
    const int t = threadIdx.x;
    if (d.k == 0) return;                        // a progressive file: pscan_kernel's
    if ((d.nc == 4) != (NS == 4)) return;        // the other instantiation's
    if (status[blockIdx.x] != 0) return;         // restart markers out of order: the segment table is not valid (uniform: before any barrier)
    const uint8_t* un = ws + d.ent.ws_unst;
    const int* seg = reinterpret_cast<const int*>(ws + d.ent.ws_seg);
    const int ns = d.nc, bpm = d.bpm, mcux = d.mcux;

    // tables
    if (t < 2 * ns) {
        const int sc = t < ns ? t : t - ns;
        const HuffSpec* hs = t < ns ? &d.dc[sc < 3 ? sc : 0] : &d.ac[sc < 3 ? sc : 0];
        if (NS == 4 && sc == 3) {
            const JExt* x = reinterpret_cast<const JExt*>(ws + d.ws_ext);
            hs = t < ns ? &x->dc : &x->ac;
        }
        lut_codes(*hs, luts[t < ns ? t : NS + t - ns]);
    }
    if (t < bpm) {
        const int sc = d.blk_comp[t], f = d.scomp[sc];
        const bool luma = d.nc > 1 && f == 0;
        s_bi[t] = BlkInfo{sc, d.blk_dx[t], d.blk_dy[t], luma ? d.hs : 1, luma ? d.vs : 1, d.bw[f], d.ws_coef[f]};
    }
    if (t < 64) s_zz[t] = kZigzag[t];
    if (t == 0) s_flags = 0;
    __syncthreads();
    for (int q = t; q < 2 * ns * (1 << LUT_BITS); q += HT) {
        const int tb = q >> LUT_BITS, e = q & ((1 << LUT_BITS) - 1);
        Lut& L = luts[tb < ns ? tb : NS + tb - ns];
        L.lut[e] = lut_entry(L, e);
    }
    __syncthreads();
    const Lut* dl = luts;
    const Lut* al = luts + NS;
    int flags = 0;
    const int k = d.k;
    const long nmcu = (long)mcux * d.mcuy;
    const long cap = d.ent.unst_cap;

    if (k == 1) {
        // every segment is one chunk with an exact start: each thread decodes whole segments
        for (int s = t; s < d.ent.nseg; s += HT) {
            const int s0 = s ? seg[s - 1] : 0, s1 = seg[s];
            if (s0 > s1) { flags |= ST_RST; continue; }
            Reader rd{un, cap, s1 * 8, -1000, 0};
            DecState st{s0 * 8, 0, 0};
            const long m0 = (long)s * d.ent.ri, m1 = m0 + d.ent.ri < nmcu ? m0 + d.ent.ri : nmcu;
            const long want = (m1 - m0) * bpm;
            int dcs[NS] = {}, pred[NS] = {}, f = 0;
            const int nb = decode_run(s_bi, bpm, mcux, s_zz, dl, al, rd, st, -1, (int)want, dcs, &f, ws, m0 * bpm, m1 * bpm, pred);
            flags |= f;
            if (nb != want || st.p > rd.E) flags |= ST_EOD;
        }
    } else {
        const int nch = d.ent.nseg * k;          // <= HT
        const int s = t / k, j = t % k;
        const bool mine = t < nch;
        int c0 = 0, c1 = 0, E = 0;
        s_cnt[t] = 0;
#pragma unroll
        for (int c = 0; c < NS; ++c) s_dc[t][c] = 0;
        if (mine) {
            const int s0 = s ? seg[s - 1] : 0, s1 = seg[s];
            const int len = s1 > s0 ? s1 - s0 : 0;
            const int L = (len + k - 1) / k;
            c0 = s0 + j * L < s1 ? s0 + j * L : s1;
            c1 = j == k - 1 ? s1 : (s0 + (j + 1) * L < s1 ? s0 + (j + 1) * L : s1);
            E = s1 * 8;
            if (s0 > s1) flags |= ST_RST;
            s_np[t] = c0 * 8;
            s_nz[t] = 0;
            s_nb[t] = 0;
            s_ep[t] = -1;
            s_need[t] = 1;
        }
        // self-synchronisation: at most k rounds (each one makes one more chunk of every segment exact)
        bool converged = false;
        for (int round = 0; round <= k; ++round) {
            if (t == 0) s_any = 0;
            __syncthreads();
            if (mine && s_need[t] && j != k - 1) {
                Reader rd{un, cap, E, -1000, 0};
                DecState st{s_np[t], s_nz[t], s_nb[t]};
                int dcs[NS] = {}, f = 0;
                const int nb = decode_run(s_bi, bpm, mcux, s_zz, dl, al, rd, st, c1 * 8, 0x7fffffff, dcs, &f, nullptr, 0, 0, nullptr);
                s_cnt[t] = nb;
#pragma unroll
                for (int c = 0; c < NS; ++c) s_dc[t][c] = dcs[c];
                if (st.p != s_ep[t] || st.z != s_ez[t] || st.b != s_eb[t]) {
                    s_ep[t] = st.p;
                    s_ez[t] = st.z;
                    s_eb[t] = st.b;
                    s_any = 1;
                }
            }
            __syncthreads();
            if (!s_any) {
                converged = true;
                break;
            }
            if (mine) {
                s_need[t] = 0;
                if (j > 0 && (s_ep[t - 1] != s_np[t] || s_ez[t - 1] != s_nz[t] || s_eb[t - 1] != s_nb[t])) {
                    s_np[t] = s_ep[t - 1];
                    s_nz[t] = s_ez[t - 1];
                    s_nb[t] = s_eb[t - 1];
                    s_need[t] = 1;
                }
            }
            __syncthreads();
        }
        if (!converged) flags |= ST_COUNT;
        // first block and DC predictors of every chunk: an exclusive scan of the block counts and DC sums over the chunks before it in its segment
        // (segmented Hillis-Steele: chunk t - o is in the same segment iff j >= o; the last chunk's own sums are 0 and nothing follows it)
        const int own0 = s_cnt[t];
        int own[NS];
#pragma unroll
        for (int c = 0; c < NS; ++c) own[c] = s_dc[t][c];
        for (int o = 1; o < HT; o <<= 1) {
            const bool take = mine && j >= o;
            int a0 = 0, a[NS] = {};
            if (take) {
                a0 = s_cnt[t - o];
#pragma unroll
                for (int c = 0; c < NS; ++c) a[c] = s_dc[t - o][c];
            }
            __syncthreads();
            if (take) {
                s_cnt[t] += a0;
#pragma unroll
                for (int c = 0; c < NS; ++c) s_dc[t][c] += a[c];
            }
            __syncthreads();
        }
        // the final pass
        if (mine) {
            const long first = s_cnt[t] - own0;
            int pred[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) pred[c] = s_dc[t][c] - own[c];
            const long m0 = (long)s * d.ent.ri, m1 = m0 + d.ent.ri < nmcu ? m0 + d.ent.ri : nmcu;
            const long want = (m1 - m0) * bpm;
            Reader rd{un, cap, E, -1000, 0};
            DecState st{s_np[t], s_nz[t], s_nb[t]};
            int dcs[NS] = {}, f = 0;
            // every chunk stops at the segment's last block: the chunk that completes it must not have read past the segment's end, and the last
            // chunk must complete it (a chunk past the data's end may have counted blocks in the padding: its successors then have nothing left)
            const long left = want - first;
            if (left > 0) {
                const int nb = decode_run(s_bi, bpm, mcux, s_zz, dl, al, rd, st, j == k - 1 ? -1 : c1 * 8, (int)left, dcs, &f, ws, m0 * bpm + first,
                                          m1 * bpm, pred);
                if ((nb == left && st.p > E) || (j == k - 1 && nb != left)) flags |= ST_EOD;
                flags |= f;
            }
        }
    }
    if (flags) atomicOr(&s_flags, flags);
    __syncthreads();
    if (t == 0 && s_flags) atomicOr(status + blockIdx.x, s_flags);
}

// ------------------------------------------------------------------------------------------------------------------------------ progressive scans
// jdphuff.c
// One restart interval (scan MCUs [m0, m1), bits from p) of one scan, by one lane.  Returns the status flags.  Whatever the bits are, block indices
// stay below the scan's host-validated MCU count and coefficient indices inside [Ss, Se]; anything libjpeg would only warn about is a flag (the host
// then decodes the file).  blk: 64 int16 of LDS of this lane (AC refinement reads the block's earlier coefficients through it).
__device__ int pscan_segment(const JDesc& d, const PScan& sc, const Lut* __restrict__ luts, const int* __restrict__ zz, Reader& rd, int p, long m0,
                             long m1, uint8_t* __restrict__ ws, int16_t* blk) {
    const int al = sc.al, ss = sc.ss, se = sc.se;
    if (ss == 0) {
        // DC: first scan (Huffman-coded difference, predictor per component, stored << Al) or refinement (one raw bit per block)
        int pr0 = 0, pr1 = 0, pr2 = 0;
        for (long m = m0; m < m1; ++m) {
            for (int i = 0; i < sc.ns; ++i) {
                const int c = sc.comp[i];
                int H = 1, V = 1;
                long bx0, by0;
                if (sc.ns == 1) {
                    bx0 = m % sc.gw;
                    by0 = m / sc.gw;
                } else {
                    const bool luma = d.nc == 3 && c == 0;
                    H = luma ? d.hs : 1;
                    V = luma ? d.vs : 1;
                    bx0 = (m % d.mcux) * H;
                    by0 = (m / d.mcux) * V;
                }
                int16_t* base = reinterpret_cast<int16_t*>(ws + d.ws_coef[c]);
                for (int y = 0; y < V; ++y)
                    for (int x = 0; x < H; ++x) {
                        int16_t* bp = base + ((by0 + y) * d.bw[c] + bx0 + x) * 64;
                        if (p > rd.E) return ST_EOD;
                        const uint32_t w32 = rd.peek32(p);
                        if (sc.ah == 0) {
                            int sym = 0;
                            const int len = huff_symbol(luts[i], w32, sym);
                            if (!len) return ST_CODE;
                            const int s = sym & 15;
                            const int v = s ? extend((int)((w32 << len) >> (32 - s)), s) : 0;
                            p += len + s;
                            int pr = i == 0 ? pr0 : (i == 1 ? pr1 : pr2);
                            pr += v;
                            if (i == 0) pr0 = pr;
                            else if (i == 1) pr1 = pr;
                            else pr2 = pr;
                            bp[0] = (int16_t)(pr * (1 << al));
                        } else {
                            if (w32 >> 31) bp[0] = (int16_t)(bp[0] | (1 << al));
                            p += 1;
                        }
                    }
            }
        }
        return p > rd.E ? ST_EOD : 0;
    }
    const int c = sc.comp[0];
    int16_t* base = reinterpret_cast<int16_t*>(ws + d.ws_coef[c]);
    const long bw = d.bw[c];
    int eobrun = 0;
    if (sc.ah == 0) {
        // AC first: run / size symbols, EOB runs across blocks, ZRL; values stored << Al
        for (long m = m0; m < m1; ++m) {
            if (eobrun > 0) {
                --eobrun;
                continue;
            }
            int16_t* bp = base + ((m / sc.gw) * bw + m % sc.gw) * 64;
            for (int k = ss; k <= se; ++k) {
                if (p > rd.E) return ST_EOD;
                const uint32_t w32 = rd.peek32(p);
                int sym = 0;
                const int len = huff_symbol(luts[0], w32, sym);
                if (!len) return ST_CODE;
                const int r = sym >> 4, s = sym & 15;
                if (s) {
                    k += r;
                    if (k > se) return ST_INDEX;
                    const int v = extend((int)((w32 << len) >> (32 - s)), s);
                    p += len + s;
                    bp[zz[k]] = (int16_t)(v * (1 << al));
                } else if (r == 15) {
                    k += 15;
                    p += len;
                } else {
                    eobrun = 1 << r;
                    if (r) eobrun += (int)((w32 << len) >> (32 - r));
                    p += len + r;
                    --eobrun;
                    break;
                }
            }
        }
        return p > rd.E ? ST_EOD : 0;
    }
    // AC refinement (decode_mcu_AC_refine): a correction bit for every already-nonzero coefficient the run passes over, new coefficients +-(1 << Al),
    // EOB runs still refine the rest of the band.  The block's 64 coefficients are read once (registers -> this lane's LDS copy for the few that
    // are corrected) and their nonzero-ness kept as a bit mask in zigzag order, so that a zero costs no memory access.  Only coefficients of the
    // band are written back, one by one: scans of the same round own other coefficients of the same blocks.
    const int p1 = 1 << al, m1v = -p1;
    for (long m = m0; m < m1; ++m) {
        int16_t* gp = base + ((m / sc.gw) * bw + m % sc.gw) * 64;        // 128-byte aligned, as blk is 16-byte aligned
        uint64_t nz = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {          // 8 bytes at a time; memcpy, so that the int16 reads below see these stores
            uint64_t v;
            __builtin_memcpy(&v, gp + 4 * q, 8);
            __builtin_memcpy(blk + 4 * q, &v, 8);
#pragma unroll
            for (int u = 0; u < 4; ++u) nz |= (uint64_t)(((v >> (16 * u)) & 0xffff) != 0) << kUnzigzag.v[4 * q + u];
        }
        auto correct = [&](int k) {             // the correction bit of the nonzero coefficient at zigzag index k
            const uint32_t bit = rd.peek32(p) >> 31;
            ++p;
            if (bit) {
                const int at = zz[k];
                const int cur = blk[at];
                if ((cur & p1) == 0) gp[at] = (int16_t)(cur >= 0 ? cur + p1 : cur + m1v);
            }
        };
        int k = ss;
        if (eobrun == 0) {
            for (; k <= se; ++k) {
                if (p > rd.E) return ST_EOD;
                const uint32_t w32 = rd.peek32(p);
                int sym = 0;
                const int len = huff_symbol(luts[0], w32, sym);
                if (!len) return ST_CODE;
                int r = sym >> 4;
                const int s = sym & 15;
                int nv = 0;
                if (s) {
                    if (s != 1) return ST_CODE;
                    nv = ((w32 << len) >> 31) ? p1 : m1v;
                    p += len + 1;
                } else if (r != 15) {
                    eobrun = 1 << r;
                    if (r) eobrun += (int)((w32 << len) >> (32 - r));
                    p += len + r;
                    break;
                } else {
                    p += len;
                }
                do {
                    if ((nz >> k) & 1) correct(k);
                    else if (--r < 0) break;
                    ++k;
                } while (k <= se);
                if (s) {
                    if (k > se) return ST_INDEX;
                    gp[zz[k]] = (int16_t)nv;
                }
            }
        }
        if (eobrun > 0) {
            if (k <= se) {
                uint64_t rest = (nz >> k) << k;                         // the nonzero coefficients of [k, se]
                if (se < 63) rest &= (1ull << (se + 1)) - 1;
                while (rest) {
                    correct(__builtin_ctzll(rest));
                    rest &= rest - 1;
                }
            }
            --eobrun;
        }
        if (p > rd.E) return ST_EOD;
    }
    return 0;
}

constexpr int PT = 64;      // threads of pscan_kernel's workgroups: one wave per scan, one lane per restart interval at a time

// grid: the scans of one launch round (scans that touch the same coefficients of a component run in different rounds, in file order).  A scan without
// restart markers is one lane's; a lane's loops run over the scan's MCUs and bands, and the reader returns zeros past its interval's end.
__global__ __launch_bounds__(PT) void pscan_kernel(const JDesc* __restrict__ descs, const PScan* __restrict__ scans, uint8_t* __restrict__ ws,
                                                   int* __restrict__ status) {
    __shared__ Lut luts[3];
    __shared__ int s_zz[64];
    // every lane's block copy starts in the same LDS bank: lanes of a file with restart markers conflict on the copy (a pitch of 68 would spread them)
    __shared__ __align__(16) int16_t s_blk[PT][64];
    __shared__ int s_skip;
    const PScan& sc = scans[blockIdx.x];
    const JDesc& d = descs[sc.img];
    const int t = threadIdx.x;
    if (t == 0) s_skip = status[sc.img];        // a file that has already failed is the host's: one read, so that the whole wave agrees
    const int ntab = sc.ss == 0 ? (sc.ah == 0 ? sc.ns : 0) : 1;
    if (t < ntab) {
        lut_codes(sc.tab[t], luts[t]);
    }
    s_zz[t] = kZigzag[t];
    __syncthreads();
    if (s_skip != 0) return;
    for (int q = t; q < ntab * (1 << LUT_BITS); q += PT) {
        Lut& L = luts[q >> LUT_BITS];
        const int e = q & ((1 << LUT_BITS) - 1);
        L.lut[e] = lut_entry(L, e);
    }
    __syncthreads();
    const uint8_t* un = ws + sc.ent.ws_unst;
    const int* seg = reinterpret_cast<const int*>(ws + sc.ent.ws_seg);
    int flags = 0;
    for (int s = t; s < sc.ent.nseg; s += PT) {
        const int s0 = s ? seg[s - 1] : 0, s1 = seg[s];
        if (s0 > s1) {
            flags |= ST_RST;
            continue;
        }
        Reader rd{un, sc.ent.unst_cap, s1 * 8, -1000, 0};
        const long m0 = (long)s * sc.ent.ri, m1 = m0 + sc.ent.ri < sc.nmcu ? m0 + sc.ent.ri : sc.nmcu;
        flags |= pscan_segment(d, sc, luts, s_zz, rd, s0 * 8, m0, m1, ws, s_blk[t]);
    }
    if (flags) atomicOr(status + sc.img, flags);
}

// jidctint.c constants (CONST_BITS 13)
#define F0298 2446
#define F0390 3196
#define F0541 4433
#define F0765 6270
#define F0899 7373
#define F1175 9633
#define F1501 12299
#define F1847 15137
#define F1961 16069
#define F2053 16819
#define F2562 20995
#define F3072 25172

__device__ inline void idct1d(int s0, int s1, int s2, int s3, int s4, int s5, int s6, int s7, int* o, int shift) {
    const int bias = 1 << (shift - 1);
    int z1 = (s2 + s6) * F0541;
    const int tmp2 = z1 + s6 * (-F1847), tmp3 = z1 + s2 * F0765;
    const int tmp0 = (s0 + s4) * 8192, tmp1 = (s0 - s4) * 8192;
    const int t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
    int o0 = s7, o1 = s5, o2 = s3, o3 = s1;
    z1 = o0 + o3;
    int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
    const int z5 = (z3 + z4) * F1175;
    o0 *= F0298;
    o1 *= F2053;
    o2 *= F3072;
    o3 *= F1501;
    z1 *= -F0899;
    z2 *= -F2562;
    z3 = z3 * -F1961 + z5;
    z4 = z4 * -F0390 + z5;
    o0 += z1 + z3;
    o1 += z2 + z4;
    o2 += z2 + z3;
    o3 += z1 + z4;
    o[0] = (t10 + o3 + bias) >> shift;
    o[7] = (t10 - o3 + bias) >> shift;
    o[1] = (t11 + o2 + bias) >> shift;
    o[6] = (t11 - o2 + bias) >> shift;
    o[2] = (t12 + o1 + bias) >> shift;
    o[5] = (t12 - o1 + bias) >> shift;
    o[3] = (t13 + o0 + bias) >> shift;
    o[4] = (t13 - o0 + bias) >> shift;
}

__device__ inline uint8_t idct_limit(int v) {
    const int x = v & 1023;
    return (uint8_t)(x < 128 ? x + 128 : (x < 512 ? 255 : (x < 896 ? 0 : x - 896)));
}

// grid (blocks / 64, B): one thread per block of every component
__global__ __launch_bounds__(64) void idct_kernel(const JDesc* __restrict__ descs, uint8_t* __restrict__ ws) {
    const JDesc& d = descs[blockIdx.y];
    long i = (long)blockIdx.x * 64 + threadIdx.x;
    int c = 0;
    for (; c < d.nc; ++c) {
        const long n = (long)d.bw[c] * d.bh[c];
        if (i < n) break;
        i -= n;
    }
    if (c >= d.nc) return;
    const int16_t* cf = reinterpret_cast<const int16_t*>(ws + d.ws_coef[c]) + i * 64;
    const uint16_t* q = c < 3 ? d.qt[c] : reinterpret_cast<const JExt*>(ws + d.ws_ext)->qt;
    int ws8[64];
#pragma unroll
    for (int u = 0; u < 8; ++u) {          // pass 1: column u
        int o[8];
        idct1d(cf[u] * q[u], cf[8 + u] * q[8 + u], cf[16 + u] * q[16 + u], cf[24 + u] * q[24 + u], cf[32 + u] * q[32 + u], cf[40 + u] * q[40 + u],
               cf[48 + u] * q[48 + u], cf[56 + u] * q[56 + u], o, 11);
#pragma unroll
        for (int y = 0; y < 8; ++y) ws8[y * 8 + u] = o[y];
    }
    const long bx = i % d.bw[c], by = i / d.bw[c];
    const long pw = (long)d.bw[c] * 8;
    uint8_t* out = ws + d.ws_plane[c] + by * 8 * pw + bx * 8;
#pragma unroll
    for (int y = 0; y < 8; ++y) {          // pass 2: row y
        int o[8];
        idct1d(ws8[y * 8], ws8[y * 8 + 1], ws8[y * 8 + 2], ws8[y * 8 + 3], ws8[y * 8 + 4], ws8[y * 8 + 5], ws8[y * 8 + 6], ws8[y * 8 + 7], o, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            lo |= (uint32_t)idct_limit(o[x]) << (8 * x);
            hi |= (uint32_t)idct_limit(o[x + 4]) << (8 * x);
        }
        uint32_t* row = reinterpret_cast<uint32_t*>(out + y * pw);     // planes are 256-aligned, pw and bx * 8 multiples of 8
        row[0] = lo;
        row[1] = hi;
    }
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sample (x, y) of the upsampled plane of a component behind the first (chroma, K): jdsample.c's fancy upsampling h2v1 / h2v2 (edges replicated at
// dw x dh; plain replication for dw <= 2) and h1v2 (whatever dw is), plain replication for 4x1 and 1x4
__device__ inline int chroma(const uint8_t* p, long pw, int x, int y, int hs, int vs, int dw, int dh) {
    if (hs == 1) {
        if (vs == 1) return p[(long)y * pw + x];
        if (vs == 4) return p[(long)(y >> 2) * pw + x];
        const int ry = y >> 1;
        const int ny = (y & 1) ? clampi(ry + 1, 0, dh - 1) : clampi(ry - 1, 0, dh - 1);
        return (3 * p[(long)ry * pw + x] + p[(long)ny * pw + x] + ((y & 1) ? 2 : 1)) >> 2;
    }
    if (hs == 4) return p[(long)y * pw + (x >> 2)];
    const int i = x >> 1;
    const int ry = vs == 2 ? y >> 1 : y;
    if (dw <= 2) return p[(long)ry * pw + i];
    const int in = (x & 1) ? clampi(i + 1, 0, dw - 1) : clampi(i - 1, 0, dw - 1);
    if (vs == 1) {
        const uint8_t* r = p + (long)ry * pw;
        return (x & 1) ? (3 * r[i] + r[in] + 2) >> 2 : (3 * r[i] + r[in] + 1) >> 2;
    }
    const int ny = (y & 1) ? clampi(ry + 1, 0, dh - 1) : clampi(ry - 1, 0, dh - 1);
    const uint8_t* r0 = p + (long)ry * pw;
    const uint8_t* r1 = p + (long)ny * pw;
    const int cs = 3 * r0[i] + r1[i], cn = 3 * r0[in] + r1[in];
    return (x & 1) ? (3 * cs + cn + 7) >> 4 : (3 * cs + cn + 8) >> 4;
}

// Pillow's MULDIV255: a * b / 255, rounded
__device__ inline int muldiv255(int a, int b) {
    const int t = a * b + 128;
    return ((t >> 8) + t) >> 8;
}

// grid (ceil(max w / 256), max h, B)
__global__ __launch_bounds__(256) void color_kernel(const JDesc* __restrict__ descs, const uint8_t* __restrict__ ws, uint8_t* __restrict__ out) {
    const JDesc& d = descs[blockIdx.z];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= d.w || y >= d.h) return;
    const long pw0 = (long)d.bw[0] * 8;
    const int Y = ws[d.ws_plane[0] + (long)y * pw0 + x];
    uint8_t* o = out + d.out + ((long)y * d.w + x) * 3;
    if (d.nc == 1) {
        o[0] = o[1] = o[2] = (uint8_t)Y;
        return;
    }
    const long pwc = (long)d.bw[1] * 8;
    const int c1 = chroma(ws + d.ws_plane[1], pwc, x, y, d.hs, d.vs, d.dw, d.dh);
    const int c2 = chroma(ws + d.ws_plane[2], pwc, x, y, d.hs, d.vs, d.dw, d.dh);
    int r = Y, g = c1, b = c2;          // CT_RGB: the planes as they are
    if (d.ct == CT_YCC || d.ct == CT_YCCK) {
        const int cb = c1 - 128, cr = c2 - 128;
        // jdcolor.c: FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554, ONE_HALF = 32768
        r = clampi(Y + ((91881 * cr + 32768) >> 16), 0, 255);
        g = clampi(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0, 255);
        b = clampi(Y + ((116130 * cb + 32768) >> 16), 0, 255);
    }
    if (d.nc == 4) {
        // libjpeg's C, M, Y are the planes (CMYK) or 255 - R, 255 - G, 255 - B (YCCK), its K the fourth plane; Pillow inverts all four and
        // convert("RGB") gives clip(nk - MULDIV255(c, nk)) with nk = 255 - k: in libjpeg's values, nk = K and c = 255 - C
        const int k = chroma(ws + d.ws_plane[3], pwc, x, y, d.hs, d.vs, d.dw, d.dh);
        if (d.ct == CT_CMYK) {
            r = 255 - r;
            g = 255 - g;
            b = 255 - b;
        }
        r = clampi(k - muldiv255(r, k), 0, 255);
        g = clampi(k - muldiv255(g, k), 0, 255);
        b = clampi(k - muldiv255(b, k), 0, 255);
    }
    o[0] = (uint8_t)r;
    o[1] = (uint8_t)g;
    o[2] = (uint8_t)b;
}

}  // namespace

extern "C" int lpi_jpeg_info_x(int flags, const void* data, long nbytes, long* info) {
    if (!data || !info || nbytes < 0 || (flags & ~LPI_JPEG_FLAGS)) return LPI_EINVAL;
    Header hd;
    if (parse_headers(static_cast<const uint8_t*>(data), nbytes, hd, flags) != 0) return LPI_EINVAL;
    info[0] = hd.gpu ? 1 : 0;
    info[1] = hd.w;
    info[2] = hd.h;
    info[3] = hd.nc;
    const bool sampled = hd.nc == 3 || (hd.nc == 4 && (flags & LPI_JPEG_LAYOUTS));
    info[4] = sampled ? hd.ch[0] : 1;
    info[5] = sampled ? hd.cv[0] : 1;
    info[6] = hd.ri;
    info[7] = hd.ent;
    info[8] = hd.prog ? 1 : 0;
    info[9] = hd.prog ? (long)hd.scans.size() : (hd.ent ? 1 : 0);
    return 0;
}

extern "C" int lpi_jpeg_info(const void* data, long nbytes, long* info) {
    long x[LPI_JPEG_INFO_X];
    if (!info) return LPI_EINVAL;
    const int rc = lpi_jpeg_info_x(0, data, nbytes, x);
    if (rc == 0) std::memcpy(info, x, LPI_JPEG_INFO * sizeof(long));
    return rc;
}

extern "C" int lpi_jpeg_decode_workspace_x(int flags, int B, const void* host, const long* offsets, long* bytes) {
    if (!bytes) return LPI_EINVAL;
    Plan pl;
    const int rc = plan(flags, B, static_cast<const uint8_t*>(host), offsets, pl);
    if (rc == 0) *bytes = pl.bytes;
    return rc;
}

extern "C" int lpi_jpeg_decode_workspace(int B, const void* host, const long* offsets, long* bytes) {
    return lpi_jpeg_decode_workspace_x(0, B, host, offsets, bytes);
}

extern "C" int lpi_jpeg_decode_u8_x(int flags, int B, const void* host, const long* offsets, const void* src, long src_bytes, const long* out_off,
                                    void* out, long out_bytes, int* status, void* ws, long ws_bytes, void* stream) {
    if (!src || !out || !status || !ws || !out_off || src_bytes < 1 || out_bytes < 1) return LPI_EINVAL;
    Plan pl;
    const int rc = plan(flags, B, static_cast<const uint8_t*>(host), offsets, pl);
    if (rc != 0) return rc;
    if (ws_bytes < pl.bytes || offsets[B] > src_bytes) return LPI_EINVAL;
    std::vector<JDesc>& descs = pl.descs;
    const std::vector<PScan>& scans = pl.scans;
    int maxw = 1, maxh = 1;
    long maxblk = 1;
    for (int i = 0; i < B; ++i) {
        JDesc& j = descs[i];
        if (out_off[i] < 0 || out_off[i] > out_bytes - (long)j.w * j.h * 3) return LPI_EINVAL;
        j.out = out_off[i];
        maxw = j.w > maxw ? j.w : maxw;
        maxh = j.h > maxh ? j.h : maxh;
        long nb = 0;
        for (int c = 0; c < j.nc; ++c) nb += (long)j.bw[c] * j.bh[c];
        maxblk = nb > maxblk ? nb : maxblk;
    }
    if (maxh > 65535 || (maxblk + 63) / 64 > 0x7fffffffL || scans.size() > 0x7fffffffUL) return LPI_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(ws, descs.data(), (size_t)B * sizeof(JDesc), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return (int)e;
    if (!scans.empty()) {
        e = hipMemcpyAsync(static_cast<char*>(ws) + pl.ws_scans, scans.data(), scans.size() * sizeof(PScan), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return (int)e;
    }
    if (!pl.exts.empty()) {
        e = hipMemcpyAsync(static_cast<char*>(ws) + pl.ws_exts, pl.exts.data(), pl.exts.size() * sizeof(JExt), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return (int)e;
    }
    e = hipMemsetAsync(static_cast<char*>(ws) + pl.zero_lo, 0, (size_t)(pl.zero_hi - pl.zero_lo), s);
    if (e != hipSuccess) return (int)e;
    const JDesc* dd = static_cast<const JDesc*>(ws);
    uint8_t* w8 = static_cast<uint8_t*>(ws);
    LPI_LAUNCH(unstuff_kernel, dim3(B), dim3(NT), 0, s, dd, (const uint8_t*)src, w8, status);
    LPI_CHECK_LAST();
    LPI_LAUNCH(huff_kernel<3>, dim3(B), dim3(HT), 0, s, dd, w8, status);
    LPI_CHECK_LAST();
    if (!pl.exts.empty()) {
        LPI_LAUNCH(huff_kernel<4>, dim3(B), dim3(HT), 0, s, dd, w8, status);
        LPI_CHECK_LAST();
    }
    if (!scans.empty()) {
        // progressive files: their scans' bytes unstuffed, then one launch per round of scans that may run side by side
        const PScan* ps = reinterpret_cast<const PScan*>(w8 + pl.ws_scans);
        LPI_LAUNCH(punstuff_kernel, dim3((unsigned)scans.size()), dim3(NT), 0, s, ps, (const uint8_t*)src, w8, status);
        LPI_CHECK_LAST();
        size_t first = 0;
        for (int r = 1; r <= LPI_JPEG_MAX_SCANS; ++r) {
            if (!pl.rounds[r]) continue;
            LPI_LAUNCH(pscan_kernel, dim3((unsigned)pl.rounds[r]), dim3(PT), 0, s, dd, ps + first, w8, status);
            LPI_CHECK_LAST();
            first += (size_t)pl.rounds[r];
        }
    }
    LPI_LAUNCH(idct_kernel, dim3((unsigned)((maxblk + 63) / 64), B), dim3(64), 0, s, dd, w8);
    LPI_CHECK_LAST();
    LPI_LAUNCH(color_kernel, dim3((maxw + 255) / 256, maxh, B), dim3(256), 0, s, dd, (const uint8_t*)w8, (uint8_t*)out);
    LPI_CHECK_LAST();
    return 0;
}

extern "C" int lpi_jpeg_decode_u8(int B, const void* host, const long* offsets, const void* src, long src_bytes, const long* out_off, void* out,
                                  long out_bytes, int* status, void* ws, long ws_bytes, void* stream) {
    return lpi_jpeg_decode_u8_x(0, B, host, offsets, src, src_bytes, out_off, out, out_bytes, status, ws, ws_bytes, stream);
}

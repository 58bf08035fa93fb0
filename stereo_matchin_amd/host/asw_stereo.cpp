// asw_stereo — command-line host driver: the reference main.cpp's ASW flow on the
// MI355X library, through the C-ABI of include/asw.h only.
//
// Mirrors stereo_matching/main.cpp:
//   * pics.txt lists image paths, two per pair (left, right) (main.cpp:136-147);
//     the output folder of a pair is its left path up to the first '/'
//     (main.cpp:150-155);
//   * images are decoded to RGBA8 (lodepng::decode in the reference,
//     main.cpp:183-186; png_io.cpp here);
//   * every pair runs `runs` times (main.cpp:213: 10) and the per-stage times of
//     each run go to a TSV file named after the device (main.cpp:164-166, 181,
//     634-708), here from HIP events (asw_timings);
//   * outputs: <folder>/asw_consistency_pre-reff.png (the reference's file of the
//     same name, main.cpp:625-627), asw_consistency.png (its `consistency_error`
//     image before refinement), asw_wta_disparity.png (its `asw_left_wta` image)
//     and, with the k = 6 refinement iterations of main.cpp:540-617 (--refine K,
//     0 = off), asw_disparity.png (refined + 3x3 median, main.cpp:619-623) and
//     asw_consistency_post-reff.png (main.cpp:629-631); where the 8-bit loop is not built
//     (D > 256 or --native-lr) the native loop on disparity indices runs instead
//     (asw_set_refine_native) and writes 16-bit images: asw_disparity16.png (refined + 3x3
//     median) and asw_consistency_post16.png (65535 = inconsistent);
//   * errors are printed and the driver continues with the next pair, like ErCheck
//     (main.cpp:27-30);
//   * beyond the reference: --devices I,J,... splits the disparity range of every
//     pair across several GPUs (asw_create_multi: RCCL all-reduces for the WTA; a
//     repeated id puts several shards on one GPU), and 16-bit disparity images
//     (asw_wta_disparity16.png, asw_consistency16.png with 65535 = inconsistent) are
//     written with --png16 and always when D > 256, where the 8-bit codes collide
//     (the LR check then compares indices, ASW_LR_NATIVE);
//   * --subpixel writes the float sub-pixel disparity of the left view
//     (asw_set_subpixel): asw_disparity_sub.pfm (one-channel PFM, the LR-masked map
//     with +inf where the check fails, the Middlebury convention; the unmasked map
//     with --no-lr) and asw_disparity_sub16.png (16-bit grey, round(64 * the
//     hole-filled map); the unmasked map with --no-lr), for D <= 1024;
//   * --cross runs the reference's first method, the cross-based matcher of
//     main.cpp:243-411 (asw_set_cross), ahead of the ASW stages of every run and writes
//     its three images (main.cpp:357-367): cross_based_initial.png,
//     cross_based_disparity.png and median.png; its timing columns (main.cpp:394-411)
//     then stand in front of the ASW columns of every TSV row, after the id and followed by
//     two empty columns, as in the reference's files.  Without --cross the files and the
//     TSV are unchanged;
//   * --census replaces the AD raw cost by the census / AD-census cost (asw_set_census;
//     --census-win WxH, --census-weights A,C: w_a * min(AD, tau) + w_c * hamming, A = 0 is
//     census only).  The outputs and the TSV columns are unchanged; the `aggr` column then
//     holds the time of the two transforms and the census cost;
//   * --sgm aggregates by semi-global matching (asw_set_sgm; --sgm-paths 4|8,
//     --sgm-penalties P1,P2) in place of the supports and the ASW passes: --taps and --iters
//     are then not read.  The outputs and the TSV columns are unchanged; `total aggregation`
//     then holds the SGM launches, supp_w and the two pass means are 0;
//   * --speckle runs the speckle filter (asw_set_speckle; --speckle-size N, --speckle-diff N)
//     on the pre-refinement left map and writes asw_speckle16.png (16-bit grey, the disparity
//     index, 65535 where the component is smaller than N pixels or the LR check fails); with
//     --subpixel also asw_disparity_sub_speckle.pfm and asw_disparity_sub_speckle16.png, the
//     --subpixel files under the filter's mask.  Every other file and the TSV are unchanged.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "asw.h"
#include "png_io.h"

using asw_host::Image;

namespace {

struct Options {
    std::string pics = "pics.txt";
    std::string root;  // default: directory of pics
    std::string tsv;   // default: "<device name>.tsv" in the current directory
    int runs = 10, ndisp = 61, taps = 33, iters = 7, device = 0, refine = 6;
    std::vector<int> devices;  // --devices: one context over several GPUs
    float gamma_c = -1.0f, gamma_g = -1.0f, tau = -1.0f;
    bool lab = false, lr = true, native_lr = false, png16 = false, subpixel = false;
    bool cross = false;  // --cross: the cross-based matcher first (main.cpp:243-411)
    int cross_arm = -1, cross_tau = -1;
    bool census = false;  // --census: the census / AD-census cost (asw_set_census)
    int census_w = -1, census_h = -1, census_ad = -1, census_wc = -1;
    bool sgm = false;  // --sgm: semi-global matching in place of the ASW passes (asw_set_sgm)
    bool sgm_paths_given = false, sgm_penalties_given = false;  // any integer reaches asw_set_sgm
    int sgm_paths = 0, sgm_p1 = 0, sgm_p2 = 0;
    bool speckle = false;  // --speckle: the speckle filter on the left map (asw_set_speckle)
    bool speckle_size_given = false, speckle_diff_given = false;  // any integer reaches asw_set_speckle
    int speckle_size = 0, speckle_diff = 0;
};

void usage() {
    std::fprintf(stderr,
                 "usage: asw_stereo [--pics FILE] [--root DIR] [--runs N] [--ndisp D] [--taps T] [--iters R]\n"
                 "                  [--gamma-c G] [--gamma-g G] [--tau TAU] [--lab] [--no-lr] [--native-lr]\n"
                 "                  [--refine K] [--device I | --devices I,J,...] [--png16] [--tsv FILE]\n"
                 "                  [--subpixel] [--cross [--cross-arm N] [--cross-tau N]]\n"
                 "                  [--census [--census-win WxH] [--census-weights A,C]]\n"
                 "                  [--sgm [--sgm-paths 4|8] [--sgm-penalties P1,P2]]\n"
                 "                  [--speckle [--speckle-size N] [--speckle-diff N]]\n"
                 "  --speckle   speckle filter on the left map: components of 4-neighbours that differ by at most\n"
                 "              --speckle-diff (default 1) and hold fewer than --speckle-size pixels (default 32) are\n"
                 "              removed: asw_speckle16.png (16-bit index, 65535 = removed or inconsistent; --ndisp <= 65535);\n"
                 "              with --subpixel also asw_disparity_sub_speckle.pfm and asw_disparity_sub_speckle16.png\n"
                 "  --refine K  refinement iterations + 3x3 median (default 6, 0 = off): asw_disparity.png and\n"
                 "              asw_consistency_post-reff.png; with --ndisp > 256 or --native-lr the loop runs on disparity\n"
                 "              indices and writes asw_disparity16.png and asw_consistency_post16.png (65535 = inconsistent)\n"
                 "  --census    the census / AD-census cost A * min(AD, tau) + C * hamming in place of the AD raw cost\n"
                 "              (robust to a gain / offset between the views); window W, H in 3, 5, 7, 9 but 9x9\n"
                 "              (default 9x7), weights A 0..64, C 1..1024 (default 1,8; A = 0: census only)\n"
                 "  --sgm       semi-global matching on the integer raw cost in place of the supports and the ASW passes\n"
                 "              (--taps and --iters are not read): 4 or 8 paths (default 8), penalties\n"
                 "              0 <= P1 <= P2 <= 1048576 (default 16,128); one GPU\n"
                 "  --cross     the reference's cross-based matcher first (one GPU, --ndisp <= 256): cross_based_initial.png,\n"
                 "              cross_based_disparity.png, median.png, and its timing columns in front of the ASW columns of the TSV\n"
                 "  --subpixel  float sub-pixel disparity (needs --ndisp <= 1024): asw_disparity_sub.pfm (LR-masked,\n"
                 "              +inf = inconsistent) and asw_disparity_sub16.png (16-bit, 64 x the hole-filled map)\n");
}

bool parse(int argc, char **argv, Options &o) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&](const char *what) -> const char * {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "%s needs a value\n", what);
                return nullptr;
            }
            return argv[++i];
        };
        const char *v = nullptr;
        if (a == "--pics") { if (!(v = next("--pics"))) return false; o.pics = v; }
        else if (a == "--root") { if (!(v = next("--root"))) return false; o.root = v; }
        else if (a == "--refine") { if (!(v = next("--refine"))) return false; o.refine = std::atoi(v); }
        else if (a == "--tsv") { if (!(v = next("--tsv"))) return false; o.tsv = v; }
        else if (a == "--runs") { if (!(v = next("--runs"))) return false; o.runs = std::atoi(v); }
        else if (a == "--ndisp") { if (!(v = next("--ndisp"))) return false; o.ndisp = std::atoi(v); }
        else if (a == "--taps") { if (!(v = next("--taps"))) return false; o.taps = std::atoi(v); }
        else if (a == "--iters") { if (!(v = next("--iters"))) return false; o.iters = std::atoi(v); }
        else if (a == "--device") { if (!(v = next("--device"))) return false; o.device = std::atoi(v); }
        else if (a == "--gamma-c") { if (!(v = next("--gamma-c"))) return false; o.gamma_c = (float)std::atof(v); }
        else if (a == "--gamma-g") { if (!(v = next("--gamma-g"))) return false; o.gamma_g = (float)std::atof(v); }
        else if (a == "--tau") { if (!(v = next("--tau"))) return false; o.tau = (float)std::atof(v); }
        else if (a == "--devices") {
            if (!(v = next("--devices"))) return false;
            o.devices.clear();
            for (const char *q = v; *q;) {
                char *end = nullptr;
                const long d = std::strtol(q, &end, 10);
                if (end == q) return false;
                o.devices.push_back((int)d);
                q = *end == ',' ? end + 1 : end;
            }
        }
        else if (a == "--png16") o.png16 = true;
        else if (a == "--subpixel") o.subpixel = true;
        else if (a == "--cross") o.cross = true;
        else if (a == "--cross-arm") { if (!(v = next("--cross-arm"))) return false; o.cross_arm = std::atoi(v); }
        else if (a == "--cross-tau") { if (!(v = next("--cross-tau"))) return false; o.cross_tau = std::atoi(v); }
        else if (a == "--census") o.census = true;
        else if (a == "--census-win") {
            if (!(v = next("--census-win"))) return false;
            if (std::sscanf(v, "%dx%d", &o.census_w, &o.census_h) != 2) return false;
            o.census = true;
        }
        else if (a == "--census-weights") {
            if (!(v = next("--census-weights"))) return false;
            if (std::sscanf(v, "%d,%d", &o.census_ad, &o.census_wc) != 2) return false;
            o.census = true;
        }
        else if (a == "--sgm") o.sgm = true;
        else if (a == "--sgm-paths") {
            if (!(v = next("--sgm-paths"))) return false;
            char tail = 0;
            if (std::sscanf(v, "%d%c", &o.sgm_paths, &tail) != 1) return false;
            o.sgm = o.sgm_paths_given = true;
        }
        else if (a == "--sgm-penalties") {
            if (!(v = next("--sgm-penalties"))) return false;
            char tail = 0;
            if (std::sscanf(v, "%d,%d%c", &o.sgm_p1, &o.sgm_p2, &tail) != 2) return false;
            o.sgm = o.sgm_penalties_given = true;
        }
        else if (a == "--speckle") o.speckle = true;
        else if (a == "--speckle-size") {
            if (!(v = next("--speckle-size"))) return false;
            char tail = 0;
            if (std::sscanf(v, "%d%c", &o.speckle_size, &tail) != 1) return false;
            o.speckle = o.speckle_size_given = true;
        }
        else if (a == "--speckle-diff") {
            if (!(v = next("--speckle-diff"))) return false;
            char tail = 0;
            if (std::sscanf(v, "%d%c", &o.speckle_diff, &tail) != 1) return false;
            o.speckle = o.speckle_diff_given = true;
        }
        else if (a == "--lab") o.lab = true;
        else if (a == "--no-lr") o.lr = false;
        else if (a == "--native-lr") o.native_lr = true;
        else if (a == "-h" || a == "--help") { usage(); std::exit(0); }
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return false; }
    }
    if (o.runs < 1) o.runs = 1;
    if (o.subpixel && o.ndisp > 1024) {  // 64 * (D - 1) must fit the 16-bit image
        std::fprintf(stderr, "--subpixel needs --ndisp <= 1024\n");
        return false;
    }
    return true;
}

std::string dir_of(const std::string &path) {
    const size_t k = path.find_last_of('/');
    return k == std::string::npos ? std::string(".") : path.substr(0, k);
}

std::string join(const std::string &a, const std::string &b) {
    if (b.empty() || b[0] == '/') return b;
    return a.empty() || a == "." ? b : a + "/" + b;
}

bool read_pairs(const std::string &path, std::vector<std::string> &left, std::vector<std::string> &right) {
    FILE *fp = std::fopen(path.c_str(), "r");
    if (!fp) return false;
    std::vector<std::string> items;
    char buf[4096];
    while (std::fscanf(fp, "%4095s", buf) == 1) items.emplace_back(buf);
    std::fclose(fp);
    for (size_t i = 0; i + 1 < items.size(); i += 2) {
        left.push_back(items[i]);
        right.push_back(items[i + 1]);
    }
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    Options o;
    if (!parse(argc, argv, o)) {
        usage();
        return 2;
    }
    if (asw_abi_version() != ASW_ABI_VERSION) {  // asw_outputs / asw_timings layouts (include/asw.h)
        std::fprintf(stderr, "libasw_hip.so has ABI revision %d, asw_stereo was built for %d: rebuild\n",
                     asw_abi_version(), ASW_ABI_VERSION);
        return 1;
    }
    if (o.root.empty()) o.root = dir_of(o.pics);
    std::vector<std::string> lefts, rights;
    if (!read_pairs(o.pics, lefts, rights)) {
        std::fprintf(stderr, "cannot read %s\n", o.pics.c_str());
        return 1;
    }
    if (o.devices.empty()) o.devices.push_back(o.device);
    char devname[256] = "hip-device";
    asw_device_name(o.devices[0], devname, (int)sizeof devname);
    if (o.devices.size() > 1) {
        const size_t k = std::strlen(devname);
        std::snprintf(devname + k, sizeof devname - k, " x%zu", o.devices.size());
    }
    std::printf("\t- Device name: %s\n", devname);
    const std::string tsv_path = o.tsv.empty() ? std::string(devname) + ".tsv" : o.tsv;
    FILE *tsv = std::fopen(tsv_path.c_str(), "w");
    if (!tsv) std::fprintf(stderr, "cannot write %s (timings go to stdout only)\n", tsv_path.c_str());

    int failures = 0;
    for (size_t k = 0; k < lefts.size(); ++k) {
        const std::string folder = lefts[k].substr(0, lefts[k].find('/'));
        std::printf("\n%s\n", folder.c_str());
        Image L, R;
        std::string e = asw_host::png_load(join(o.root, lefts[k]), L);
        if (e.empty()) e = asw_host::png_load(join(o.root, rights[k]), R);
        if (e.empty() && (L.width != R.width || L.height != R.height)) e = "left and right sizes differ";
        if (!e.empty()) {
            std::fprintf(stderr, "%s: %s\n", folder.c_str(), e.c_str());
            ++failures;
            continue;
        }
        asw_params p;
        asw_params_default(&p);
        p.width = (int)L.width;
        p.height = (int)L.height;
        p.ndisp = o.ndisp;
        p.taps = o.taps;
        p.iters = o.iters;
        if (o.gamma_c > 0) p.gamma_c = o.gamma_c;
        if (o.gamma_g > 0) p.gamma_g = o.gamma_g;
        if (o.tau > 0) p.tad_tau = o.tau;
        p.color_space = o.lab ? ASW_COLOR_LAB : ASW_COLOR_RGB;
        p.lr_check = o.lr ? 1 : 0;
        const bool wide = p.ndisp > 256;  // 8-bit codes collide: compare indices, write 16-bit images
        p.lr_mode = (o.native_lr || wide) ? ASW_LR_NATIVE : ASW_LR_U8;
        const bool png16 = o.png16 || wide;
        asw_ctx *ctx = nullptr;
        int st = o.devices.size() > 1 ? asw_create_multi(&p, o.devices.data(), (int)o.devices.size(), &ctx)
                                      : asw_create(&p, o.devices[0], &ctx);
        if (st != ASW_OK) {
            std::fprintf(stderr, "%s: asw_create: %s (hip %d)\n", folder.c_str(), asw_strerror(st),
                         asw_last_hip_error());
            ++failures;
            continue;
        }
        // the loop runs on d-sharded contexts too (asw_set_refine: its asw_WTA_REF scan is
        // exchanged like the WTA); it feeds back 8-bit codes, so D > 256 and the native LR
        // rule take the native loop on indices (asw_set_refine_native, 16-bit images)
        const bool native = p.lr_mode == ASW_LR_NATIVE;
        const bool refine = o.refine > 0 && p.lr_check && !native;
        const bool nrefine = o.refine > 0 && p.lr_check && native;
        if (o.refine > 0 && !p.lr_check)
            std::fprintf(stderr, "%s: refinement skipped (it needs the LR check)\n", folder.c_str());
        if (refine) {
            asw_refine_params rp;
            asw_refine_params_default(&rp);
            rp.iters = o.refine;
            st = asw_set_refine(ctx, &rp);
            if (st != ASW_OK) {
                std::fprintf(stderr, "%s: asw_set_refine: %s\n", folder.c_str(), asw_strerror(st));
                ++failures;
                asw_destroy(ctx);
                continue;
            }
        }
        const size_t S = (size_t)p.width * p.height;
        std::vector<uint16_t> fin16(nrefine ? S : 0), post16(nrefine ? S : 0);
        if (nrefine) {  // registered once, filled by every asw_match
            asw_refine_params rp;
            asw_refine_params_default(&rp);
            rp.iters = o.refine;
            asw_refine_native_outputs no;
            std::memset(&no, 0, sizeof no);
            no.final16 = fin16.data();
            no.post16 = post16.data();
            st = asw_set_refine_native(ctx, &rp, &no);
            if (st != ASW_OK) {
                std::fprintf(stderr, "%s: asw_set_refine_native: %s\n", folder.c_str(), asw_strerror(st));
                ++failures;
                asw_destroy(ctx);
                continue;
            }
        }
        if (o.census) {
            asw_census_params np;
            asw_census_params_default(&np);
            if (o.census_w >= 0) np.win_w = o.census_w, np.win_h = o.census_h;
            if (o.census_ad >= 0) np.ad_weight = o.census_ad, np.census_weight = o.census_wc;
            st = asw_set_census(ctx, &np);
            if (st != ASW_OK) {
                std::fprintf(stderr, "%s: asw_set_census: %s\n", folder.c_str(), asw_strerror(st));
                ++failures;
                asw_destroy(ctx);
                continue;
            }
        }
        if (o.sgm) {  // after the census switch: the check needs the cost SGM will read
            asw_sgm_params sp;
            asw_sgm_params_default(&sp);
            if (o.sgm_paths_given) sp.paths = o.sgm_paths;
            if (o.sgm_penalties_given) sp.p1 = o.sgm_p1, sp.p2 = o.sgm_p2;
            st = asw_set_sgm(ctx, &sp);
            if (st != ASW_OK) {
                std::fprintf(stderr, "%s: asw_set_sgm: %s\n", folder.c_str(), asw_strerror(st));
                ++failures;
                asw_destroy(ctx);
                continue;
            }
        }
        std::vector<uint8_t> disp(S * 4), lr(S * 4), lr_red(S * 4), fin(S * 4), post(S * 4);
        std::vector<uint16_t> disp16(png16 ? S : 0), lr16(png16 ? S : 0);
        // sub-pixel float maps: registered once, filled by every asw_match
        std::vector<float> sub(o.subpixel ? S : 0), sub_lr(o.subpixel && p.lr_check ? S : 0),
            sub_fill(o.subpixel && p.lr_check ? S : 0);
        if (o.subpixel) {
            asw_subpixel_outputs so;
            so.disp = sub.data();
            so.disp_lr = p.lr_check ? sub_lr.data() : nullptr;
            so.disp_filled = p.lr_check ? sub_fill.data() : nullptr;
            st = asw_set_subpixel(ctx, &so);
            if (st != ASW_OK) {
                std::fprintf(stderr, "%s: asw_set_subpixel: %s\n", folder.c_str(), asw_strerror(st));
                ++failures;
                asw_destroy(ctx);
                continue;
            }
        }
        // speckle filter: registered once, run after the consistency stage by every asw_match
        const bool spk_sub = o.speckle && o.subpixel;
        std::vector<uint16_t> spk16(o.speckle ? S : 0);
        std::vector<float> spk_lr(spk_sub ? S : 0), spk_fill(spk_sub ? S : 0);
        if (o.speckle) {
            asw_speckle_params kp;
            asw_speckle_params_default(&kp);
            if (o.speckle_size_given) kp.min_size = o.speckle_size;
            if (o.speckle_diff_given) kp.max_diff = o.speckle_diff;
            asw_speckle_outputs ko;
            std::memset(&ko, 0, sizeof ko);
            ko.filtered16 = spk16.data();
            ko.disp_lr = spk_sub ? spk_lr.data() : nullptr;
            ko.disp_filled = spk_sub ? spk_fill.data() : nullptr;
            st = asw_set_speckle(ctx, &kp, &ko);
            if (st != ASW_OK) {
                std::fprintf(stderr, "%s: asw_set_speckle: %s\n", folder.c_str(), asw_strerror(st));
                ++failures;
                asw_destroy(ctx);
                continue;
            }
        }
        // cross-based matcher: registered once, run ahead of the ASW stages by every asw_match
        std::vector<uint8_t> cr_init(o.cross ? S * 4 : 0), cr_fin(o.cross ? S * 4 : 0), cr_med(o.cross ? S * 4 : 0);
        asw_cross_timings ct;
        std::memset(&ct, 0, sizeof ct);
        if (o.cross) {
            asw_cross_params cp;
            asw_cross_params_default(&cp);
            if (o.cross_arm >= 0) cp.arm_max = o.cross_arm;
            if (o.cross_tau >= 0) cp.tau = o.cross_tau;
            asw_cross_outputs co;
            std::memset(&co, 0, sizeof co);
            co.initial_rgba = cr_init.data();
            co.final_rgba = cr_fin.data();
            co.median_left_rgba = cr_med.data();
            co.timings = &ct;
            st = asw_set_cross(ctx, &cp, &co);
            if (st != ASW_OK) {
                std::fprintf(stderr, "%s: asw_set_cross: %s\n", folder.c_str(), asw_strerror(st));
                ++failures;
                asw_destroy(ctx);
                continue;
            }
        }
        asw_outputs out;
        std::memset(&out, 0, sizeof out);
        out.disp_rgba = disp.data();
        out.lr_rgba = lr.data();
        out.lr_red_rgba = lr_red.data();
        out.final_rgba = refine ? fin.data() : nullptr;
        out.post_red_rgba = refine ? post.data() : nullptr;
        out.disp16 = png16 ? disp16.data() : nullptr;
        out.lr16 = png16 && p.lr_check ? lr16.data() : nullptr;
        if (tsv) {
            std::fprintf(tsv, "\n%s - %s\n", devname, folder.c_str());
            // --cross: the cross columns of main.cpp:394-411 between the id and the ASW columns,
            // under the reference's own column names and with its two empty columns after them
            std::fprintf(tsv, "id\t");
            if (o.cross)
                std::fprintf(tsv, "medL_solo\tmedR_solo\tmed_full\tcross_h\tcross_v\tcross_full\taggregation\tintegral_h\t"
                                  "aggr_h\tintegral_v\taggr_v\tinit_disp\tfinal_disp\tcross method total\t\t\t");
            std::fprintf(tsv, "aggr\tsupp_w\tv_aggr_mean\th_aggr_mean\ttotal aggregation\twta\tconsistency\t"
                              "total\trefine\th2d\td2h\texchange\n");
        }
        for (int run = 0; run < o.runs && st == ASW_OK; ++run) {
            asw_timings t;
            std::memset(&t, 0, sizeof t);
            st = asw_match(ctx, L.rgba.data(), R.rgba.data(), &out, &t);
            if (st != ASW_OK) break;
            std::printf("run %d: total %.3f ms (aggregation %.3f, V %.3f, H %.3f per pass)\n", run, t.total,
                        t.aggregation_total, t.v_pass_mean, t.h_pass_mean);
            if (tsv) std::fprintf(tsv, "%d\t", run);
            if (tsv && o.cross)
                std::fprintf(tsv, "%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t"
                                  "%0.3f\t%0.3f\t\t\t",
                             ct.median[0], ct.median[1], ct.median[0] + ct.median[1], ct.cross[0], ct.cross[1],
                             ct.cross[0] + ct.cross[1], ct.aggregation, ct.integral_h, ct.oii_h, ct.integral_v,
                             ct.oii_v, ct.init, ct.vote, ct.total);
            if (tsv)
                std::fprintf(tsv, "%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\t%0.3f\n",
                             t.raw_cost, t.support, t.v_pass_mean, t.h_pass_mean, t.aggregation_total, t.wta,
                             t.consistency, t.total, t.refine, t.h2d, t.d2h, t.exchange);
        }
        asw_destroy(ctx);
        if (st != ASW_OK) {
            std::fprintf(stderr, "%s: asw_match: %s (hip %d)\n", folder.c_str(), asw_strerror(st),
                         asw_last_hip_error());
            ++failures;
            continue;
        }
        const std::string dir = join(o.root, folder);
        struct {
            const char *name;
            const std::vector<uint8_t> *img;
        } outs[] = {{"asw_wta_disparity.png", &disp},
                    {"asw_consistency.png", &lr},
                    {"asw_consistency_pre-reff.png", &lr_red},
                    {"asw_disparity.png", &fin},
                    {"asw_consistency_post-reff.png", &post}};
        for (const auto &w : outs) {
            if (!p.lr_check && w.img != &disp) continue;
            if (!refine && (w.img == &fin || w.img == &post)) continue;
            e = asw_host::png_save(dir + "/" + w.name, w.img->data(), L.width, L.height, 4);
            if (!e.empty()) {
                std::fprintf(stderr, "%s: %s\n", folder.c_str(), e.c_str());
                ++failures;
            }
        }
        if (o.cross) {  // main.cpp:357-367
            e = asw_host::png_save(dir + "/cross_based_initial.png", cr_init.data(), L.width, L.height, 4);
            if (e.empty()) e = asw_host::png_save(dir + "/cross_based_disparity.png", cr_fin.data(), L.width, L.height, 4);
            if (e.empty()) e = asw_host::png_save(dir + "/median.png", cr_med.data(), L.width, L.height, 4);
            if (!e.empty()) {
                std::fprintf(stderr, "%s: %s\n", folder.c_str(), e.c_str());
                ++failures;
            }
        }
        if (png16) {
            e = asw_host::png_save16(dir + "/asw_wta_disparity16.png", disp16.data(), L.width, L.height);
            if (e.empty() && p.lr_check)
                e = asw_host::png_save16(dir + "/asw_consistency16.png", lr16.data(), L.width, L.height);
            if (!e.empty()) {
                std::fprintf(stderr, "%s: %s\n", folder.c_str(), e.c_str());
                ++failures;
            }
        }
        if (nrefine) {
            e = asw_host::png_save16(dir + "/asw_disparity16.png", fin16.data(), L.width, L.height);
            if (e.empty())
                e = asw_host::png_save16(dir + "/asw_consistency_post16.png", post16.data(), L.width, L.height);
            if (!e.empty()) {
                std::fprintf(stderr, "%s: %s\n", folder.c_str(), e.c_str());
                ++failures;
            }
        }
        if (o.subpixel) {
            // PFM: the LR-masked map, invalid = +inf; PNG: round-to-nearest(64 * dense map)
            std::vector<float> &pf = p.lr_check ? sub_lr : sub;
            const std::vector<float> &dense = p.lr_check ? sub_fill : sub;
            for (float &v : pf)
                if (v != v) v = INFINITY;
            std::vector<uint16_t> q(S);
            for (size_t i = 0; i < S; ++i) q[i] = (uint16_t)std::nearbyintf(dense[i] * 64.0f);
            e = asw_host::pfm_save(dir + "/asw_disparity_sub.pfm", pf.data(), L.width, L.height);
            if (e.empty()) e = asw_host::png_save16(dir + "/asw_disparity_sub16.png", q.data(), L.width, L.height);
            if (!e.empty()) {
                std::fprintf(stderr, "%s: %s\n", folder.c_str(), e.c_str());
                ++failures;
            }
        }
        if (o.speckle) {
            e = asw_host::png_save16(dir + "/asw_speckle16.png", spk16.data(), L.width, L.height);
            if (e.empty() && spk_sub) {  // the encodings of the --subpixel files
                for (float &v : spk_lr)
                    if (v != v) v = INFINITY;
                std::vector<uint16_t> q(S);
                for (size_t i = 0; i < S; ++i) q[i] = (uint16_t)std::nearbyintf(spk_fill[i] * 64.0f);
                e = asw_host::pfm_save(dir + "/asw_disparity_sub_speckle.pfm", spk_lr.data(), L.width, L.height);
                if (e.empty())
                    e = asw_host::png_save16(dir + "/asw_disparity_sub_speckle16.png", q.data(), L.width, L.height);
            }
            if (!e.empty()) {
                std::fprintf(stderr, "%s: %s\n", folder.c_str(), e.c_str());
                ++failures;
            }
        }
    }
    if (tsv) std::fclose(tsv);
    return failures ? 1 : 0;
}

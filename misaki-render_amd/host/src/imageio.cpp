// imageio.cpp — float image output for HDRFilm::develop (the reference goes through OpenImageIO,
// src/librender/image.cpp:20-43): PFM and uncompressed scanline OpenEXR (32-bit float channels); image input for the
// `bitmap` texture and the `envmap` emitter: PFM, Radiance RGBE (.hdr) and binary PGM / PPM.
#include <misaki/render.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>

namespace misaki {

void write_pfm(const std::string &path, int w, int h, int channels, const float *data) {
    if (channels != 1 && channels != 3) Throw("write_pfm(): 1 or 3 channels expected");
    std::ofstream os(path, std::ios::binary);
    if (!os) Throw("Could not open \"{}\" for writing", path);
    os << (channels == 3 ? "PF" : "Pf") << "\n" << w << " " << h << "\n-1.0\n";   // little endian, bottom-up rows
    for (int y = h - 1; y >= 0; --y) os.write((const char *) (data + (size_t) y * w * channels), (std::streamsize) sizeof(float) * w * channels);
}

namespace {
// one header token of a PNM / PFM file: whitespace and '#' comments skipped; empty at the end of the file
std::string header_token(std::istream &is) {
    std::string t;
    int c;
    while ((c = is.get()) != EOF) {
        if (c == '#') { while ((c = is.get()) != EOF && c != '\n') {} continue; }
        if (!std::isspace(c)) { t.push_back((char) c); break; }
    }
    while ((c = is.get()) != EOF && !std::isspace(c)) t.push_back((char) c);      // (consumes the ONE whitespace after the token)
    return t;
}
// IEC 61966-2-1: encoded value in [0, 1] -> linear, in double, rounded once
float srgb_to_linear(double v) { return (float) (v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4)); }
// Radiance RGBE (.hdr): "#?RADIANCE" / "#?RGBE", header lines up to an empty one, "-Y H +X W", then H scanlines, each flat
// (W x 4 bytes) or run-length encoded per channel (2 2 W_hi W_lo, then per channel counts > 128 = a run, <= 128 = literals; only
// for 8 <= W < 32768).  A pixel (r, g, b, e) is (m + 0.5) * 2^(e - 136) per channel, 0 for e == 0.
void read_hdr(std::istream &is, const std::string &path, int &w, int &h, std::vector<float> &rgb) {
    std::string line;
    bool format_seen = false;
    std::getline(is, line);                                        // the magic line (checked by the caller)
    while (std::getline(is, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) break;
        if (line.compare(0, 7, "FORMAT=") == 0) {
            format_seen = true;
            if (line != "FORMAT=32-bit_rle_rgbe") Throw("\"{}\": Radiance image with {} is not supported (32-bit_rle_rgbe only)", path, line);
        }
    }
    if (!is) Throw("\"{}\": truncated or invalid image header", path);
    (void) format_seen;                                            // (a file without a FORMAT line is rgbe by definition)
    if (!std::getline(is, line)) Throw("\"{}\": truncated or invalid image header", path);
    if (!line.empty() && line.back() == '\r') line.pop_back();
    long lh = 0, lw = 0;
    char sy[3] = "", sx[3] = "", tail = 0;
    if (std::sscanf(line.c_str(), "%2s %ld %2s %ld %c", sy, &lh, sx, &lw, &tail) != 4)
        Throw("\"{}\": truncated or invalid image header (resolution \"{}\")", path, line);
    if (std::strcmp(sy, "-Y") != 0 || std::strcmp(sx, "+X") != 0)
        Throw("\"{}\": Radiance image orientation \"{}\" is not supported (-Y H +X W only)", path, line);
    if (lw < 1 || lh < 1 || lw > 65536 || lh > 65536) Throw("\"{}\": truncated or invalid image header (resolution \"{}\")", path, line);
    w = (int) lw; h = (int) lh;
    rgb.assign((size_t) w * h * 3, 0.f);
    std::vector<unsigned char> scan((size_t) w * 4);
    auto need = [&](unsigned char *dst, size_t n) {
        is.read((char *) dst, (std::streamsize) n);
        if ((size_t) is.gcount() != n) Throw("\"{}\": truncated image file (scanline data)", path);
    };
    for (int y = 0; y < h; ++y) {
        unsigned char head[4];
        need(head, 4);
        const bool rle = w >= 8 && w < 32768 && head[0] == 2 && head[1] == 2 && !(head[2] & 0x80);
        if (rle) {
            if (((int) head[2] << 8 | head[3]) != w) Throw("\"{}\": run-length encoded scanline {} has length {}, the image is {} wide", path, y, (int) head[2] << 8 | head[3], w);
            for (int c = 0; c < 4; ++c) {
                int x = 0;
                while (x < w) {
                    unsigned char cnt, val;
                    need(&cnt, 1);
                    if (cnt > 128) {
                        const int run = cnt - 128;
                        need(&val, 1);
                        if (x + run > w) Throw("\"{}\": run-length encoded scanline {} overruns the image width", path, y);
                        for (int k = 0; k < run; ++k) scan[(size_t) (x++) * 4 + c] = val;
                    } else {
                        if (cnt == 0 || x + cnt > w) Throw("\"{}\": run-length encoded scanline {} overruns the image width", path, y);
                        for (int k = 0; k < cnt; ++k) { need(&val, 1); scan[(size_t) (x++) * 4 + c] = val; }
                    }
                }
            }
        } else {
            std::memcpy(scan.data(), head, 4);
            if (w > 1) need(scan.data() + 4, (size_t) (w - 1) * 4);
            for (int x = 0; x < w; ++x)
                if (scan[(size_t) x * 4] == 1 && scan[(size_t) x * 4 + 1] == 1 && scan[(size_t) x * 4 + 2] == 1)
                    Throw("\"{}\": old-style run-length encoded Radiance scanlines are not supported", path);
        }
        for (int x = 0; x < w; ++x) {
            const unsigned char *p = &scan[(size_t) x * 4];
            if (p[3] == 0) continue;
            const double f = std::ldexp(1.0, (int) p[3] - 136);
            for (int c = 0; c < 3; ++c) rgb[((size_t) y * w + x) * 3 + c] = (float) (((double) p[c] + 0.5) * f);
        }
    }
}
}  // namespace

void read_image(const std::string &path, bool raw, int &w, int &h, std::vector<float> &rgb) {
    std::ifstream is(path, std::ios::binary);
    if (!is) Throw("Could not open the image file \"{}\"", path);
    {   // a Radiance file starts with "#?", which the PNM header rules would skip as a comment
        char m[11] = "";
        is.read(m, 10);
        const std::string start(m, (size_t) is.gcount());
        is.clear(); is.seekg(0);
        if (start.compare(0, 10, "#?RADIANCE") == 0 || start.compare(0, 6, "#?RGBE") == 0) { read_hdr(is, path, w, h, rgb); return; }
    }
    const std::string magic = header_token(is);
    const bool pfm = magic == "PF" || magic == "Pf", pnm = magic == "P5" || magic == "P6";
    if (!pfm && !pnm) Throw("\"{}\": not a PFM, Radiance RGBE or binary PGM / PPM image (magic number \"{}\")", path, magic.substr(0, 8));
    const int channels = (magic == "PF" || magic == "P6") ? 3 : 1;
    const std::string ws = header_token(is), hs = header_token(is), third = header_token(is);
    char *end = nullptr;
    const long lw = std::strtol(ws.c_str(), &end, 10), lh = std::strtol(hs.c_str(), nullptr, 10);
    const double scale = std::strtod(third.c_str(), &end);
    if (third.empty() || lw < 1 || lh < 1 || lw > 65536 || lh > 65536 || end == third.c_str())
        Throw("\"{}\": truncated or invalid image header", path);
    w = (int) lw; h = (int) lh;
    const size_t n = (size_t) w * h * channels;
    rgb.assign((size_t) w * h * 3, 0.f);
    auto put = [&](size_t pixel, int c, float v) { if (channels == 3) rgb[pixel * 3 + c] = v; else rgb[pixel * 3] = rgb[pixel * 3 + 1] = rgb[pixel * 3 + 2] = v; };
    if (pfm) {
        if (scale == 0.0) Throw("\"{}\": invalid PFM scale", path);
        const bool little = scale < 0.0;
        std::vector<unsigned char> buf(n * 4);
        is.read((char *) buf.data(), (std::streamsize) buf.size());
        if ((size_t) is.gcount() != buf.size()) Throw("\"{}\": truncated image file ({} of {} bytes of pixel data)", path, (size_t) is.gcount(), buf.size());
        for (size_t k = 0; k < n; ++k) {
            const unsigned char *b = &buf[k * 4];
            const uint32_t bits = little ? (uint32_t) b[0] | (uint32_t) b[1] << 8 | (uint32_t) b[2] << 16 | (uint32_t) b[3] << 24
                                         : (uint32_t) b[3] | (uint32_t) b[2] << 8 | (uint32_t) b[1] << 16 | (uint32_t) b[0] << 24;
            float v; std::memcpy(&v, &bits, 4);
            const size_t px = k / channels, row = px / w, col = px % w;
            put(((size_t) h - 1 - row) * w + col, (int) (k % channels), v);      // the file's first row is the image's bottom row
        }
        return;
    }
    const long maxval = std::strtol(third.c_str(), nullptr, 10);
    if (maxval < 1 || maxval > 65535) Throw("\"{}\": invalid maxval {}", path, third);
    const size_t bps = maxval > 255 ? 2 : 1;
    std::vector<unsigned char> buf(n * bps);
    is.read((char *) buf.data(), (std::streamsize) buf.size());
    if ((size_t) is.gcount() != buf.size()) Throw("\"{}\": truncated image file ({} of {} bytes of pixel data)", path, (size_t) is.gcount(), buf.size());
    for (size_t k = 0; k < n; ++k) {
        const unsigned v = bps == 2 ? (unsigned) buf[k * 2] << 8 | buf[k * 2 + 1] : buf[k];      // (two-byte samples: most significant first)
        const double e = (double) v / (double) maxval;
        put(k / channels, (int) (k % channels), raw ? (float) e : srgb_to_linear(e));
    }
}

void write_exr(const std::string &path, int w, int h, const std::vector<std::string> &channels, const float *data) {
    std::ofstream os(path, std::ios::binary);
    if (!os) Throw("Could not open \"{}\" for writing", path);
    auto put32 = [&](uint32_t v) { os.write((const char *) &v, 4); };
    auto put64 = [&](uint64_t v) { os.write((const char *) &v, 8); };
    auto attr = [&](const char *name, const char *type, const std::string &payload) {
        os.write(name, std::strlen(name) + 1); os.write(type, std::strlen(type) + 1);
        put32((uint32_t) payload.size()); os.write(payload.data(), (std::streamsize) payload.size());
    };
    put32(20000630u); put32(2u);                           // magic, version 2, single-part scanline
    std::vector<size_t> order(channels.size());            // channels are stored alphabetically
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return channels[a] < channels[b]; });
    std::string ch;
    for (size_t i : order) {
        ch += channels[i]; ch += '\0';
        uint32_t v[4] = {2u /* FLOAT */, 0u, 1u, 1u};       // type, pLinear + reserved, xSampling, ySampling
        ch.append((const char *) v, 16);
    }
    ch += '\0';
    attr("channels", "chlist", ch);
    attr("compression", "compression", std::string(1, '\0'));
    int32_t box[4] = {0, 0, w - 1, h - 1};
    attr("dataWindow", "box2i", std::string((const char *) box, 16));
    attr("displayWindow", "box2i", std::string((const char *) box, 16));
    attr("lineOrder", "lineOrder", std::string(1, '\0'));
    float one = 1.f, zero2[2] = {0.f, 0.f};
    attr("pixelAspectRatio", "float", std::string((const char *) &one, 4));
    attr("screenWindowCenter", "v2f", std::string((const char *) zero2, 8));
    attr("screenWindowWidth", "float", std::string((const char *) &one, 4));
    os.put('\0');
    const size_t nc = channels.size();
    const uint64_t line_bytes = (uint64_t) w * nc * 4;
    uint64_t offset = (uint64_t) os.tellp() + (uint64_t) h * 8;
    for (int y = 0; y < h; ++y) { put64(offset); offset += 8 + line_bytes; }
    std::vector<float> row((size_t) w);
    for (int y = 0; y < h; ++y) {
        put32((uint32_t) y); put32((uint32_t) line_bytes);
        for (size_t i : order) {
            for (int x = 0; x < w; ++x) row[x] = data[((size_t) y * w + x) * nc + i];
            os.write((const char *) row.data(), (std::streamsize) w * 4);
        }
    }
}

}  // namespace misaki

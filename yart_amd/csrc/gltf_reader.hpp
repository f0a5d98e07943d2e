// gltf_reader.hpp — glTF 2.0 / GLB importer producing the scene description the renderer takes
// (SURVEY §8(f) rank 1). Host only. Stands where the reference's loader stands
// (src/gltf/gltf.cpp:319-358, which sits on fastgltf — a dependency the reference does not vendor)
// and reproduces what that loader does with an asset, including the parts that are quirks:
//
//  * materials (gltf.cpp:62-176): baseColorFactor rgb, baseColorTexture as a 4-channel sRGB
//    texture, metallicRoughnessTexture reduced to channels {1, 2} (roughness, metallic),
//    KHR_materials_transmission (+ 1-channel texture) / ior / anisotropy / clearcoat (no clearcoat
//    texture) / volume (density = 1 / attenuationDistance) / emissive_strength; thin transmission
//    is forced on (:105); images are taken from buffer views only (:32-39 — an image given by URI
//    yields no texture);
//  * textures (core/texture.hpp:62-92): decoded to 4 channels, the requested channels kept;
//    sRGB-typed textures are re-encoded with gamma 2 — every kept channel, alpha included;
//  * meshes (gltf.cpp:178-270): all TRIANGLES primitives of a mesh merged into one vertex / face
//    list, material index value_or(0), NORMAL and TEXCOORD_0 required, TANGENT optional (zero);
//  * nodes (gltf.cpp:272-317): T * R * S with the half-matrix quaternion form (:6-19), the inverse
//    by the cofactor expansion of math/mat.hpp:399-536, every operation in float in source order;
//  * lights (gltf.cpp:295-314): one AreaLight per emissive triangle, children before the node
//    itself, carrying `node.transform * globalTransform`; the per-face light index restarts at 0
//    in every node (so it is an index into the node's own lights, not into the scene's list).
//
// Not taken from the asset, as in the reference: cameras, KHR_lights_punctual, texture transforms,
// samplers (wrap is always repeat), vertex colours, skins, animations, morph targets.
// Node `matrix` properties are decomposed to T / R / S first (fastgltf's DecomposeNodeMatrices
// option); that decomposition is restated from the glTF specification, so matrix-valued nodes may
// differ from the reference in the last bits of the node transform. Embedded PNG and JPEG
// images are decoded to the reference's bytes (image_decode.hpp); arithmetic-coded / CMYK JPEG and sparse
// accessors are refused with an error.
#pragma once
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "image_decode.hpp"
#include "json_mini.hpp"
#include "scene_file.hpp"

namespace yart_hip {
namespace gltf {

// ---- float 4x4 algebra exactly as the reference evaluates it --------------------------------------
struct M4 { float m[16]; };
inline M4 identity4() { M4 r{}; r.m[0] = r.m[5] = r.m[10] = r.m[15] = 1.0f; return r; }
inline M4 mul(const M4& a, const M4& b) {                 // math/mat.hpp:262-273: zero, then += in k order
  M4 r{};
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float acc = 0.0f;
      for (int k = 0; k < 4; k++) acc += a.m[i * 4 + k] * b.m[k * 4 + j];
      r.m[i * 4 + j] = acc;
    }
  return r;
}
inline M4 scale(const M4& a, float s) { M4 r; for (int i = 0; i < 16; i++) r.m[i] = a.m[i] * s; return r; }
// math/mat.hpp:399-536 (cofactor expansion, products and sums left to right, then * (1 / det))
inline bool inverse(const M4& mm, M4& out) {
  const float* m = mm.m;
  float inv[16];
  inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
  inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
  inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
  float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
  if (det == 0.0f) return false;
  det = 1.0f / det;
  for (int i = 0; i < 16; i++) out.m[i] = inv[i] * det;
  return true;
}
struct Xform { M4 fwd, inv; };                             // math/transform.hpp Transform (matrix pair)
inline Xform identityX() { return {identity4(), identity4()}; }
inline Xform compose(const Xform& a, const Xform& b) {     // transform.hpp:56-61  a * b
  return {mul(a.fwd, b.fwd), mul(b.inv, a.inv)};
}
// gltf.cpp:6-19 (quaternion x, y, z, w) and :284-289
inline M4 rotationFromQuat(const float q[4]) {
  const float qr = q[3], qi = q[0], qj = q[1], qk = q[2];
  M4 half{};
  half.m[0] = 0.5f - (qj * qj + qk * qk); half.m[1] = (qi * qj - qr * qk); half.m[2] = (qi * qk + qr * qj);
  half.m[4] = (qi * qj + qr * qk); half.m[5] = 0.5f - (qi * qi + qk * qk); half.m[6] = (qj * qk - qr * qi);
  half.m[8] = (qi * qk - qr * qj); half.m[9] = (qj * qk + qr * qi); half.m[10] = 0.5f - (qi * qi + qj * qj);
  half.m[15] = 0.5f;
  return scale(half, 2.0f);
}
inline Xform fromTRS(const float t[3], const float q[4], const float s[3]) {
  M4 T = identity4(); T.m[3] = t[0]; T.m[7] = t[1]; T.m[11] = t[2];
  M4 S = identity4(); S.m[0] = s[0]; S.m[5] = s[1]; S.m[10] = s[2];
  Xform x;
  x.fwd = mul(mul(T, rotationFromQuat(q)), S);
  if (!inverse(x.fwd, x.inv)) throw std::runtime_error("gltf: singular node transform");   // reference: optional::value() throws
  return x;
}
// column-major glTF matrix -> T, R (unit quaternion), S
inline void decomposeMatrix(const double cm[16], float t[3], float q[4], float s[3]) {
  double c[3][3];
  for (int col = 0; col < 3; col++) for (int row = 0; row < 3; row++) c[col][row] = cm[col * 4 + row];
  t[0] = float(cm[12]); t[1] = float(cm[13]); t[2] = float(cm[14]);
  double sc[3];
  for (int col = 0; col < 3; col++) sc[col] = std::sqrt(c[col][0] * c[col][0] + c[col][1] * c[col][1] + c[col][2] * c[col][2]);
  const double det = c[0][0] * (c[1][1] * c[2][2] - c[2][1] * c[1][2]) - c[1][0] * (c[0][1] * c[2][2] - c[2][1] * c[0][2]) +
                     c[2][0] * (c[0][1] * c[1][2] - c[1][1] * c[0][2]);
  if (det < 0.0) sc[0] = -sc[0];
  double r[3][3];                                            // r[row][col]
  for (int col = 0; col < 3; col++) for (int row = 0; row < 3; row++) r[row][col] = sc[col] != 0.0 ? c[col][row] / sc[col] : (row == col ? 1.0 : 0.0);
  double qx, qy, qz, qw;
  const double tr = r[0][0] + r[1][1] + r[2][2];
  if (tr > 0.0) { const double k = std::sqrt(tr + 1.0) * 2.0; qw = 0.25 * k; qx = (r[2][1] - r[1][2]) / k; qy = (r[0][2] - r[2][0]) / k; qz = (r[1][0] - r[0][1]) / k; }
  else if (r[0][0] > r[1][1] && r[0][0] > r[2][2]) { const double k = std::sqrt(1.0 + r[0][0] - r[1][1] - r[2][2]) * 2.0; qw = (r[2][1] - r[1][2]) / k; qx = 0.25 * k; qy = (r[0][1] + r[1][0]) / k; qz = (r[0][2] + r[2][0]) / k; }
  else if (r[1][1] > r[2][2]) { const double k = std::sqrt(1.0 + r[1][1] - r[0][0] - r[2][2]) * 2.0; qw = (r[0][2] - r[2][0]) / k; qx = (r[0][1] + r[1][0]) / k; qy = 0.25 * k; qz = (r[1][2] + r[2][1]) / k; }
  else { const double k = std::sqrt(1.0 + r[2][2] - r[0][0] - r[1][1]) * 2.0; qw = (r[1][0] - r[0][1]) / k; qx = (r[0][2] + r[2][0]) / k; qy = (r[1][2] + r[2][1]) / k; qz = 0.25 * k; }
  q[0] = float(qx); q[1] = float(qy); q[2] = float(qz); q[3] = float(qw);
  s[0] = float(sc[0]); s[1] = float(sc[1]); s[2] = float(sc[2]);
}

// ---- the asset -----------------------------------------------------------------------------------
inline std::vector<uint8_t> readFile(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open " + path);
  std::fseek(f, 0, SEEK_END);
  const long sz = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> d(sz > 0 ? size_t(sz) : 0);
  const size_t got = d.empty() ? 0 : std::fread(d.data(), 1, d.size(), f);
  std::fclose(f);
  if (got != d.size()) throw std::runtime_error("short read on " + path);
  return d;
}
inline std::vector<uint8_t> base64Decode(const char* s, size_t n) {
  std::vector<uint8_t> out;
  uint32_t acc = 0; int bits = 0;
  for (size_t i = 0; i < n; i++) {
    const char c = s[i];
    int v;
    if (c >= 'A' && c <= 'Z') v = c - 'A'; else if (c >= 'a' && c <= 'z') v = c - 'a' + 26;
    else if (c >= '0' && c <= '9') v = c - '0' + 52; else if (c == '+' || c == '-') v = 62; else if (c == '/' || c == '_') v = 63;
    else if (c == '=') break; else continue;
    acc = (acc << 6) | uint32_t(v); bits += 6;
    if (bits >= 8) { bits -= 8; out.push_back(uint8_t((acc >> bits) & 0xFFu)); }
  }
  return out;
}
inline std::string percentDecode(const std::string& s) {
  std::string o;
  for (size_t i = 0; i < s.size(); i++) {
    if (s[i] == '%' && i + 2 < s.size() && std::isxdigit((unsigned char) s[i + 1]) && std::isxdigit((unsigned char) s[i + 2])) {
      o.push_back(char(std::strtol(s.substr(i + 1, 2).c_str(), nullptr, 16))); i += 2;
    } else o.push_back(s[i]);
  }
  return o;
}

class Importer {
 public:
  explicit Importer(const std::string& path) : path_(path) {
    const size_t slash = path.find_last_of("/\\");
    dir_ = slash == std::string::npos ? std::string(".") : path.substr(0, slash);
    file_ = readFile(path);
    const uint8_t* jsonPtr = file_.data();
    size_t jsonLen = file_.size();
    if (file_.size() >= 12 && std::memcmp(file_.data(), "glTF", 4) == 0) {
      uint32_t version, total;
      std::memcpy(&version, &file_[4], 4); std::memcpy(&total, &file_[8], 4);
      if (version != 2) fail("GLB container version " + std::to_string(version) + " (2 expected)");
      size_t pos = 12;
      const size_t end = std::min(size_t(total), file_.size());
      jsonPtr = nullptr;
      while (pos + 8 <= end) {
        uint32_t clen, ctype;
        std::memcpy(&clen, &file_[pos], 4); std::memcpy(&ctype, &file_[pos + 4], 4);
        if (pos + 8 + size_t(clen) > end) fail("truncated GLB chunk");
        if (ctype == 0x4E4F534Au && !jsonPtr) { jsonPtr = &file_[pos + 8]; jsonLen = clen; }
        else if (ctype == 0x004E4942u && !glbBin_) { glbBin_ = &file_[pos + 8]; glbBinLen_ = clen; }
        pos += 8 + size_t(clen) + ((4 - clen % 4) % 4);
      }
      if (!jsonPtr) fail("GLB without a JSON chunk");
    }
    doc_ = json::parse(reinterpret_cast<const char*>(jsonPtr), jsonLen);
    if (!doc_.isObject()) fail("document is not an object");
    const std::string ver = doc_.get("asset").get("version").string();
    if (ver.empty() || ver[0] != '2') fail("asset.version '" + ver + "' (2.x expected)");
    for (const auto& ext : doc_.get("extensionsRequired").arr) {
      const std::string& e = ext.string();
      static const char* known[] = {"KHR_materials_emissive_strength", "KHR_materials_transmission", "KHR_materials_ior",
                                    "KHR_materials_anisotropy", "KHR_materials_clearcoat", "KHR_materials_volume"};
      bool ok = false;
      for (const char* k : known) ok = ok || e == k;
      if (!ok) fail("required extension " + e + " is not supported");        // as fastgltf's Parser refuses it
    }
    loadBuffers();
  }

  std::unique_ptr<LoadedScene> run() {
    out_ = std::make_unique<LoadedScene>();
    const json::Value& mats = doc_.get("materials");
    for (size_t i = 0; i < mats.size(); i++) out_->materials.push_back(material(mats.at(i)));
    const json::Value& meshes = doc_.get("meshes");
    for (size_t i = 0; i < meshes.size(); i++) mesh(meshes.at(i), i);
    // node 0 = root, identity (gltf.cpp:346-347)
    YartNodeDesc root{};
    root.parent = -1; root.mesh = -1;
    put(root.fwd, identity4()); put(root.inv, identity4());
    out_->nodes.push_back(root);
    const json::Value& scenes = doc_.get("scenes");
    if (scenes.size() == 0) fail("asset has no scenes");
    const size_t sceneIdx = size_t(doc_.get("scene").integer(0));
    const json::Value& sceneNodes = scenes.at(sceneIdx).get("nodes");
    for (size_t i = 0; i < sceneNodes.size(); i++) node(size_t(sceneNodes.at(i).integer(-1)));
    finish();
    return std::move(out_);
  }

 private:
  std::string path_, dir_;
  std::vector<uint8_t> file_;
  const uint8_t* glbBin_ = nullptr;
  size_t glbBinLen_ = 0;
  json::Value doc_;
  std::vector<std::vector<uint8_t>> buffers_;
  std::unique_ptr<LoadedScene> out_;
  std::map<std::pair<size_t, int>, int32_t> texCache_;
  struct MeshData { std::vector<float> pos, nrm, tan, uv; std::vector<uint32_t> faces; std::vector<int32_t> faceLight; };
  std::vector<MeshData> meshData_;

  [[noreturn]] void fail(const std::string& what) const { throw std::runtime_error("gltf (" + path_ + "): " + what); }
  static void put(float dst[16], const M4& m) { std::memcpy(dst, m.m, sizeof(float) * 16); }

  void loadBuffers() {
    const json::Value& bufs = doc_.get("buffers");
    for (size_t i = 0; i < bufs.size(); i++) {
      const json::Value& b = bufs.at(i);
      const size_t want = size_t(b.get("byteLength").integer(0));
      std::vector<uint8_t> data;
      if (!b.has("uri")) {
        if (i != 0 || !glbBin_) fail("buffer " + std::to_string(i) + " has no uri and there is no GLB binary chunk");
        data.assign(glbBin_, glbBin_ + glbBinLen_);
      } else {
        const std::string& uri = b.get("uri").string();
        if (uri.compare(0, 5, "data:") == 0) {
          const size_t comma = uri.find(',');
          if (comma == std::string::npos || uri.find(";base64") == std::string::npos) fail("buffer data URI is not base64");
          data = base64Decode(uri.c_str() + comma + 1, uri.size() - comma - 1);
        } else data = readFile(dir_ + "/" + percentDecode(uri));
      }
      if (data.size() < want) fail("buffer " + std::to_string(i) + " is shorter than its byteLength");
      buffers_.push_back(std::move(data));
    }
  }
  struct View { const uint8_t* ptr; size_t len, stride; };
  View view(int64_t idx) const {
    const json::Value& views = doc_.get("bufferViews");
    if (idx < 0 || size_t(idx) >= views.size()) fail("bufferView index out of range");
    const json::Value& v = views.at(size_t(idx));
    const int64_t b = v.get("buffer").integer(-1);
    if (b < 0 || size_t(b) >= buffers_.size()) fail("buffer index out of range");
    const size_t off = size_t(v.get("byteOffset").integer(0)), len = size_t(v.get("byteLength").integer(0));
    if (off > buffers_[size_t(b)].size() || len > buffers_[size_t(b)].size() - off) fail("bufferView exceeds its buffer");
    return {buffers_[size_t(b)].data() + off, len, size_t(v.get("byteStride").integer(0))};
  }
  // accessor -> floats (nComp per element; integer components converted, normalised ones per the specification)
  // or unsigned indices. Returns the element count.
  size_t accessor(int64_t idx, uint32_t nComp, std::vector<float>* outF, std::vector<uint32_t>* outU) const {
    const json::Value& accs = doc_.get("accessors");
    if (idx < 0 || size_t(idx) >= accs.size()) fail("accessor index out of range");
    const json::Value& a = accs.at(size_t(idx));
    if (a.has("sparse")) fail("sparse accessors are not supported");
    const std::string& type = a.get("type").string();
    const uint32_t have = type == "SCALAR" ? 1 : type == "VEC2" ? 2 : type == "VEC3" ? 3 : type == "VEC4" ? 4 : 0;
    if (have != nComp) fail("accessor " + std::to_string(idx) + " has type " + type + ", " + std::to_string(nComp) + " components expected");
    const int64_t ct = a.get("componentType").integer(0);
    const size_t csz = (ct == 5120 || ct == 5121) ? 1 : (ct == 5122 || ct == 5123) ? 2 : (ct == 5125 || ct == 5126) ? 4 : 0;
    if (!csz) fail("accessor component type " + std::to_string(ct));
    const size_t count = size_t(a.get("count").integer(0));
    const bool normalized = a.get("normalized").boolean(false);
    if (outF) outF->assign(count * nComp, 0.0f);
    if (outU) outU->assign(count * nComp, 0u);
    if (!a.has("bufferView")) return count;                      // all zeros
    const View v = view(a.get("bufferView").integer(-1));
    const size_t off = size_t(a.get("byteOffset").integer(0));
    const size_t elem = csz * nComp, stride = v.stride ? v.stride : elem;
    if (count && (off > v.len || (count - 1) * stride + elem > v.len - off)) fail("accessor " + std::to_string(idx) + " exceeds its bufferView");
    for (size_t i = 0; i < count; i++) {
      const uint8_t* p = v.ptr + off + i * stride;
      for (uint32_t c = 0; c < nComp; c++, p += csz) {
        float f = 0.0f; uint32_t u = 0;
        switch (ct) {
          case 5120: { int8_t x; std::memcpy(&x, p, 1); f = normalized ? std::fmax(float(x) / 127.0f, -1.0f) : float(x); u = uint32_t(x); break; }
          case 5121: { uint8_t x = *p; f = normalized ? float(x) / 255.0f : float(x); u = x; break; }
          case 5122: { int16_t x; std::memcpy(&x, p, 2); f = normalized ? std::fmax(float(x) / 32767.0f, -1.0f) : float(x); u = uint32_t(x); break; }
          case 5123: { uint16_t x; std::memcpy(&x, p, 2); f = normalized ? float(x) / 65535.0f : float(x); u = x; break; }
          case 5125: { uint32_t x; std::memcpy(&x, p, 4); f = float(x); u = x; break; }
          default: { std::memcpy(&f, p, 4); u = uint32_t(f); break; }
        }
        if (outF) (*outF)[i * nComp + c] = f;
        if (outU) (*outU)[i * nComp + c] = u;
      }
    }
    return count;
  }

  // core/texture.hpp:78-84: byte -> sRGB decode -> sqrt -> byte (truncated)
  static const uint8_t* gamma2Table() {
    static uint8_t table[256];
    static bool init = false;
    if (!init) {
      for (int b = 0; b < 256; b++) {
        const float in = float(b) / 255.0f;
        float val = in <= 0.04045f ? in / 12.92f : std::pow((in + 0.055f) / 1.055f, 2.4f);   // core/color-utils.hpp:12-15
        val = std::sqrt(val);
        table[b] = uint8_t(val * 255.0f);
      }
      init = true;
    }
    return table;
  }
  // textures[idx] as a C-channel texture of the given type (gltf.cpp:21-48 + texture.hpp:62-92); -1 if the
  // reference would end up without one
  int32_t texture(const json::Value& ref, uint32_t C, uint32_t type, const uint32_t channels[4], int kind) {
    if (!ref.isObject()) return -1;
    const int64_t ti = ref.get("index").integer(-1);
    const json::Value& texs = doc_.get("textures");
    if (ti < 0 || size_t(ti) >= texs.size()) fail("texture index out of range");
    const auto key = std::make_pair(size_t(ti), kind);
    const auto hit = texCache_.find(key);
    if (hit != texCache_.end()) return hit->second;
    int32_t result = -1;
    const json::Value& t = texs.at(size_t(ti));
    if (t.has("source")) {
      const int64_t ii = t.get("source").integer(-1);
      const json::Value& imgs = doc_.get("images");
      if (ii < 0 || size_t(ii) >= imgs.size()) fail("image index out of range");
      const json::Value& im = imgs.at(size_t(ii));
      if (im.has("bufferView")) {
        const View v = view(im.get("bufferView").integer(-1));
        image::Image8 img;
        try { img = image::decodeImage8(v.ptr, v.len); }
        catch (const std::exception& e) { fail("image " + std::to_string(ii) + ": " + e.what()); }
        std::vector<uint8_t> data(size_t(img.width) * img.height * C);
        const uint8_t* g2 = gamma2Table();
        for (size_t i = 0; i < size_t(img.width) * img.height; i++)
          for (uint32_t j = 0; j < C; j++) {
            uint8_t px = img.rgba[i * 4 + channels[j]];
            if (type == 1) px = g2[px];
            data[i * C + j] = px;
          }
        YartTextureDesc d{};
        d.width = img.width; d.height = img.height; d.channels = C; d.is_float = 0; d.type = type;
        out_->blobs.push_back(std::move(data));
        d.data = out_->blobs.back().data();
        out_->textures.push_back(d);
        result = int32_t(out_->textures.size() - 1);
      }
    }
    texCache_[key] = result;
    return result;
  }

  static void vec(const json::Value& v, float* dst, size_t n) {
    if (v.isArray()) for (size_t i = 0; i < n && i < v.size(); i++) dst[i] = v.at(i).numberF(dst[i]);
  }
  YartMaterialDesc material(const json::Value& m) {                       // gltf.cpp:62-176
    YartMaterialDesc d{};
    const json::Value& pbr = m.get("pbrMetallicRoughness");
    const json::Value& ext = m.get("extensions");
    float base[4] = {1, 1, 1, 1};
    vec(pbr.get("baseColorFactor"), base, 4);
    d.base[0] = base[0]; d.base[1] = base[1]; d.base[2] = base[2];
    static const uint32_t ch0123[4] = {0, 1, 2, 3}, ch12[4] = {1, 2, 0, 0};
    d.tex_base = texture(pbr.get("baseColorTexture"), 4, 1, ch0123, 0);
    d.roughness = pbr.get("roughnessFactor").numberF(1.0f);
    d.metallic = pbr.get("metallicFactor").numberF(1.0f);
    d.tex_mr = texture(pbr.get("metallicRoughnessTexture"), 2, 2, ch12, 1);
    d.transmission = 0.0f; d.tex_transmission = -1;
    const json::Value& tr = ext.get("KHR_materials_transmission");
    if (tr.isObject()) {
      d.transmission = tr.get("transmissionFactor").numberF(0.0f);
      d.tex_transmission = texture(tr.get("transmissionTexture"), 1, 2, ch0123, 2);
    }
    d.thin_transmission = 1;                                               // :105
    const json::Value& an = ext.get("KHR_materials_anisotropy");
    if (an.isObject()) { d.anisotropic = an.get("anisotropyStrength").numberF(0.0f); d.aniso_rotation = an.get("anisotropyRotation").numberF(0.0f); }
    d.clearcoat = 0.0f; d.clearcoat_roughness = 0.03f;
    const json::Value& cc = ext.get("KHR_materials_clearcoat");
    if (cc.isObject()) { d.clearcoat = cc.get("clearcoatFactor").numberF(0.0f); d.clearcoat_roughness = cc.get("clearcoatRoughnessFactor").numberF(0.0f); }
    d.tex_clearcoat = -1;
    float em[3] = {0, 0, 0};
    vec(m.get("emissiveFactor"), em, 3);
    d.tex_emission = texture(m.get("emissiveTexture"), 3, 1, ch0123, 3);
    const float strength = ext.get("KHR_materials_emissive_strength").get("emissiveStrength").numberF(1.0f);
    for (int i = 0; i < 3; i++) d.emission[i] = em[i] * strength;
    d.normal_scale = 1.0f;
    d.tex_normal = texture(m.get("normalTexture"), 3, 2, ch0123, 4);
    if (m.get("normalTexture").isObject()) d.normal_scale = m.get("normalTexture").get("scale").numberF(1.0f);
    d.volume_color[0] = d.volume_color[1] = d.volume_color[2] = 1.0f;
    d.volume_density = 0.0f;
    const json::Value& vol = ext.get("KHR_materials_volume");
    if (vol.isObject()) {
      vec(vol.get("attenuationColor"), d.volume_color, 3);
      d.volume_density = vol.has("attenuationDistance") ? 1.0f / vol.get("attenuationDistance").numberF(0.0f) : 0.0f;   // 1 / +inf
    }
    d.ior = ext.get("KHR_materials_ior").get("ior").numberF(1.5f);
    return d;
  }

  void mesh(const json::Value& gm, size_t meshIdx) {                     // gltf.cpp:178-270
    MeshData md;
    const json::Value& prims = gm.get("primitives");
    for (size_t pi = 0; pi < prims.size(); pi++) {
      const json::Value& p = prims.at(pi);
      const size_t idxOffset = md.pos.size() / 3;
      const uint32_t materialIdx = uint32_t(p.get("material").integer(0));
      if (materialIdx >= out_->materials.size()) fail("mesh " + std::to_string(meshIdx) + " uses material " + std::to_string(materialIdx) + " which the asset does not define");
      if (p.get("mode").integer(4) != 4) continue;                         // TRIANGLES only
      const json::Value& at = p.get("attributes");
      auto need = [&](const char* name) -> int64_t {
        if (!at.has(name)) fail("mesh " + std::to_string(meshIdx) + " primitive " + std::to_string(pi) + " has no " + name + " (the reference loader requires it)");
        return at.get(name).integer(-1);
      };
      std::vector<float> pos, nrm, uv, tan;
      const size_t nv = accessor(need("POSITION"), 3, &pos, nullptr);
      const size_t nn = accessor(need("NORMAL"), 3, &nrm, nullptr);
      const size_t nt = accessor(need("TEXCOORD_0"), 2, &uv, nullptr);
      nrm.resize(nv * 3, 0.0f); uv.resize(nv * 2, 0.0f);
      (void)nn; (void)nt;
      if (at.has("TANGENT")) accessor(at.get("TANGENT").integer(-1), 4, &tan, nullptr);
      tan.resize(nv * 4, 0.0f);
      md.pos.insert(md.pos.end(), pos.begin(), pos.end());
      md.nrm.insert(md.nrm.end(), nrm.begin(), nrm.end());
      md.tan.insert(md.tan.end(), tan.begin(), tan.end());
      md.uv.insert(md.uv.end(), uv.begin(), uv.end());
      std::vector<uint32_t> idx;
      if (p.has("indices")) accessor(p.get("indices").integer(-1), 1, nullptr, &idx);
      else { idx.resize(nv); for (size_t i = 0; i < nv; i++) idx[i] = uint32_t(i); }    // fastgltf GenerateMeshIndices
      for (size_t i = 0; i + 2 < idx.size(); i += 3) {
        for (int k = 0; k < 3; k++) {
          if (idx[i + k] >= nv) fail("mesh " + std::to_string(meshIdx) + " has a vertex index out of range");
          md.faces.push_back(uint32_t(idx[i + k] + idxOffset));
        }
        md.faces.push_back(materialIdx);
      }
    }
    if (md.faces.empty()) fail("mesh " + std::to_string(meshIdx) + " has no triangles");
    md.faceLight.assign(md.faces.size() / 4, -1);                          // core/mesh.hpp:47
    meshData_.push_back(std::move(md));
  }

  static bool emissive(const YartMaterialDesc& m) {                       // bsdf/parametric.cpp:66
    return m.emission[0] * m.emission[0] + m.emission[1] * m.emission[1] + m.emission[2] * m.emission[2] > 0.0f;
  }
  // gltf.cpp:272-317 (processNode) without recursion: an explicit stack of the open nodes, so that a hierarchy of any depth
  // imports without exhausting the host stack. The reference's observable order is kept: node records in pre-order,
  // localTransform = node.transform * globalTransform (:293), and a node's area lights after those of all its children
  // (:295-314: the recursion into the children comes first). A node reachable from two parents is instanced once per path,
  // as the recursion does; a node that is its own ancestor is refused (the reference would recurse until its stack runs out).
  void node(size_t rootIdx) {
    const json::Value& nodes = doc_.get("nodes");
    struct Open { size_t idx; int32_t self; int32_t mesh; Xform global; size_t next; };
    std::vector<Open> stack;
    std::vector<uint8_t> onPath(nodes.size(), 0);
    auto enter = [&](size_t nodeIdx, int32_t parent, const Xform& global) {
      if (nodeIdx >= nodes.size()) fail("node index out of range");
      if (onPath[nodeIdx]) fail("node hierarchy has a cycle: node " + std::to_string(nodeIdx) + " is its own ancestor");
      if (out_->nodes.size() >= (1u << 20) - 1u) fail("more than 2^20 scene nodes (a node shared by many parents is instanced once per path)");
      const json::Value& n = nodes.at(nodeIdx);
      float t[3] = {0, 0, 0}, q[4] = {0, 0, 0, 1}, s[3] = {1, 1, 1};
      if (n.has("matrix")) {
        double cm[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        const json::Value& mv = n.get("matrix");
        for (size_t i = 0; i < 16 && i < mv.size(); i++) cm[i] = mv.at(i).number(cm[i]);
        decomposeMatrix(cm, t, q, s);
      } else { vec(n.get("translation"), t, 3); vec(n.get("rotation"), q, 4); vec(n.get("scale"), s, 3); }
      const Xform local = fromTRS(t, q, s);
      YartNodeDesc d{};
      d.parent = parent;
      d.mesh = -1;
      if (n.has("mesh")) {
        const int64_t mi = n.get("mesh").integer(-1);
        if (mi < 0 || size_t(mi) >= meshData_.size()) fail("mesh index out of range");
        d.mesh = int32_t(mi);
      }
      put(d.fwd, local.fwd); put(d.inv, local.inv);
      const int32_t self = int32_t(out_->nodes.size());
      out_->nodes.push_back(d);
      onPath[nodeIdx] = 1;
      stack.push_back(Open{nodeIdx, self, d.mesh, compose(local, global), 0});     // :293 — node.transform * globalTransform
    };
    enter(rootIdx, 0, identityX());
    while (!stack.empty()) {
      Open& top = stack.back();
      const json::Value& ch = nodes.at(top.idx).get("children");
      if (top.next < ch.size()) {
        const size_t c = size_t(ch.at(top.next++).integer(-1));
        const Xform g = top.global;                 // (enter() may reallocate the stack)
        enter(c, top.self, g);
        continue;
      }
      const Open done = top;
      stack.pop_back();
      onPath[done.idx] = 0;
      if (done.mesh >= 0) {
        MeshData& md = meshData_[size_t(done.mesh)];
        int32_t li = 0;
        for (size_t f = 0; f < md.faceLight.size(); f++) {
          const YartMaterialDesc& mat = out_->materials[md.faces[f * 4 + 3]];
          if (!emissive(mat)) continue;
          YartLightDesc l{};
          l.type = 0; l.mesh = done.mesh; l.tri = uint32_t(f); l.two_sided = 0; l.texture = -1; l.radius = 100.0f;
          std::memcpy(l.emission, mat.emission, sizeof(l.emission));
          put(l.fwd, done.global.fwd); put(l.inv, done.global.inv);
          out_->lights.push_back(l);
          md.faceLight[f] = li++;
        }
      }
    }
  }

  void finish() {
    auto own = [&](const void* p, size_t bytes) -> const void* {
      const uint8_t* b = static_cast<const uint8_t*>(p);
      out_->blobs.emplace_back(b, b + bytes);
      return out_->blobs.back().data();
    };
    for (const MeshData& md : meshData_) {
      YartMeshDesc m{};
      m.n_vertices = uint32_t(md.pos.size() / 3); m.n_faces = uint32_t(md.faces.size() / 4);
      m.positions = static_cast<const float*>(own(md.pos.data(), md.pos.size() * 4));
      m.normals = static_cast<const float*>(own(md.nrm.data(), md.nrm.size() * 4));
      m.tangents = static_cast<const float*>(own(md.tan.data(), md.tan.size() * 4));
      m.uvs = static_cast<const float*>(own(md.uv.data(), md.uv.size() * 4));
      m.faces = static_cast<const uint32_t*>(own(md.faces.data(), md.faces.size() * 4));
      m.face_light = static_cast<const int32_t*>(own(md.faceLight.data(), md.faceLight.size() * 4));
      out_->meshes.push_back(m);
    }
    out_->refreshDesc();
  }
};

inline std::unique_ptr<LoadedScene> loadGltf(const std::string& path) { return Importer(path).run(); }

// frontend main.cpp:80-86: the environment is not part of the asset — an octahedral Radiance .hdr wrapped in an
// ImageInfiniteLight(radius, texture) (identity transform), or a UniformInfiniteLight(radius, emission), appended
// after the asset's area lights.
inline void addImageEnvironment(LoadedScene& s, const std::string& hdrPath, float radius) {
  const std::vector<uint8_t> file = readFile(hdrPath);
  const image::ImageF img = image::decodeHdr(file.data(), file.size());
  std::vector<uint8_t> data(size_t(img.width) * img.height * 3 * sizeof(float));
  float* rgb = reinterpret_cast<float*>(data.data());
  for (size_t i = 0; i < size_t(img.width) * img.height; i++) for (int c = 0; c < 3; c++) rgb[i * 3 + c] = img.rgba[i * 4 + c];   // core/texture.cpp:9-15
  YartTextureDesc t{};
  t.width = img.width; t.height = img.height; t.channels = 3; t.is_float = 1; t.type = 0;
  s.blobs.push_back(std::move(data));
  t.data = s.blobs.back().data();
  s.textures.push_back(t);
  YartLightDesc l{};
  l.type = 2; l.mesh = -1; l.texture = int32_t(s.textures.size() - 1); l.radius = radius;
  std::memcpy(l.fwd, identity4().m, sizeof(l.fwd)); std::memcpy(l.inv, identity4().m, sizeof(l.inv));
  s.lights.push_back(l);
  s.refreshDesc();
}
inline void addUniformEnvironment(LoadedScene& s, const float emission[3], float radius) {
  YartLightDesc l{};
  l.type = 1; l.mesh = -1; l.texture = -1; l.radius = radius;
  std::memcpy(l.emission, emission, sizeof(l.emission));
  std::memcpy(l.fwd, identity4().m, sizeof(l.fwd)); std::memcpy(l.inv, identity4().m, sizeof(l.inv));
  s.lights.push_back(l);
  s.refreshDesc();
}

}  // namespace gltf
}  // namespace yart_hip

// GroundingDINO engine: checkpoint (Hugging Face port's key names) -> the handle's packed weights. ovm_gdino_create (gdino.hip) calls
// load_bert, load_swin, load_neck, load_encoder, load_decoder in this order; key names, packing order and with them the order of the
// slab allocations are fixed (weight addresses relative to each other are part of what the timings were measured on).
#include <cmath>
#include "gdino_model.hpp"

namespace ovm {
namespace gdino {
namespace {

const std::string M = "model.";

int up_ln(OvmGdino* g, const WeightMap& wm, const std::string& prefix, Ln* ln) {
  OVM_TRY(g, upload_weight(g, wm, prefix + ".weight", -1, &ln->g));
  return upload_weight(g, wm, prefix + ".bias", -1, &ln->b);
}

// The row-chain kernels (dec_chain.hip) feed weight fragments from global memory straight into v_mfma_f32_16x16x32_f16: lane l wants
// row l % 16, k-chunk l / 16 of a 16-row tile - read from the row-major image that is 16 different rows per quarter-wave, 64 cache
// lines per load instruction with 16 bytes used of each (measured: ~13 us per 256 x 256 projection, 20 GB/s per CU). This copy holds
// the image in the order the lanes consume it: [tile of 16 rows][k-step of 32][hi | lo][lane 0..63][8 halves] - one load
// instruction = 1 KiB contiguous.
int make_frag(OvmGdino* g, Lin* w) {
  std::vector<half_t> src; src.swap(w->img);          // released on return
  if (g->precision != 3 || !w->hi) return OVM_OK;
  const size_t n = packed_halves(w->N, w->Kpad, 3);
  if (src.size() != n) { g->err = "make_frag: the weight was packed without keeping its host image"; return OVM_ERR_INVALID; }
  std::vector<half_t> dst(n);
  if (const int r = host_frag_order(src.data(), w->N, w->Kpad, dst.data())) { g->err = "make_frag: not a split image with Kpad % 32 == 0"; return r; }
  OVM_TRY(g, g->alloc(&w->frag, n));
  OVM_HIP(g, hipMemcpy(w->frag, dst.data(), n * sizeof(half_t), hipMemcpyHostToDevice));
  return OVM_OK;
}

// concatenation along N of several nn.Linear, shapes read off the checkpoint; keep: a make_frag of this weight follows
int pack_cat(OvmGdino* g, const WeightMap& wm, const std::vector<std::string>& prefixes, Lin* out, bool with_bias = true,
             const float* row_scale = nullptr, bool keep = false) {
  std::vector<std::pair<std::string, int>> parts;
  for (auto& p : prefixes) parts.push_back({p, -1});
  return pack_concat(g, wm, parts, -1, out, with_bias, row_scale, keep ? &out->img : nullptr);
}
int pack_lin(OvmGdino* g, const WeightMap& wm, const std::string& prefix, Lin* out, bool with_bias = true, bool keep = false) {
  return pack_cat(g, wm, {prefix}, out, with_bias, nullptr, keep);
}
// square convolution, shape read off the checkpoint
int pack_conv(OvmGdino* g, const WeightMap& wm, const std::string& prefix, Lin* out, int* ksize) {
  const OvmTensor* t; OVM_TRY(g, find_weight(g, wm, prefix + ".weight", -1, &t));
  if (t->ndim != 4) { g->err = "conv weight must be 4-d: " + prefix; return OVM_ERR_SHAPE; }
  if (ksize) *ksize = (int)t->shape[2];
  return ovm::pack_conv(g, wm, prefix, (int)t->shape[0], (int)t->shape[1], (int)t->shape[2], BIAS_REQUIRED, out);
}

int load_mha(OvmGdino* g, const WeightMap& wm, const std::string& p, int heads, Mha* m, bool cross, bool keep = false) {
  m->heads = heads;
  if (cross) {
    OVM_TRY(g, pack_lin(g, wm, p + "query", &m->q, true, keep));
  } else {
    OVM_TRY(g, pack_cat(g, wm, {p + "query", p + "key"}, &m->qk, true, nullptr, keep));
    OVM_TRY(g, pack_lin(g, wm, p + "value", &m->v, true, keep));
  }
  return pack_lin(g, wm, p + "out_proj", &m->out, true, keep);
}
int load_msda(OvmGdino* g, const WeightMap& wm, const std::string& p, MsdaW* m, bool with_value, bool keep = false) {
  OVM_TRY(g, pack_cat(g, wm, {p + "sampling_offsets", p + "attention_weights"}, &m->offw, true, nullptr, keep));
  if (with_value) OVM_TRY(g, pack_lin(g, wm, p + "value_proj", &m->value, true, keep));
  return pack_lin(g, wm, p + "output_proj", &m->out, true, keep);
}

int load_swin_block(OvmGdino* g, const WeightMap& wm, const std::string& q, int C, int nh, const std::vector<int>& rel_index, SwinBlock* blk) {
  const int ws = g->cfg.swin_window, ws2 = ws * ws;
  OVM_TRY(g, up_ln(g, wm, q + "layernorm_before", &blk->ln1));
  OVM_TRY(g, up_ln(g, wm, q + "layernorm_after", &blk->ln2));
  const bool fused = swin_qkv_attn_supported(C, nh, ws, g->precision);
  OVM_TRY(g, pack_cat(g, wm, {q + "attention.q_proj", q + "attention.k_proj", q + "attention.v_proj"}, &blk->qkv, true, nullptr, fused));
  if (fused) OVM_TRY(g, make_frag(g, &blk->qkv));      // the window kernel projects q | k | v itself
  OVM_TRY(g, pack_lin(g, wm, q + "attention.o_proj", &blk->proj));
  OVM_TRY(g, pack_lin(g, wm, q + "mlp.fc1", &blk->fc1));
  OVM_TRY(g, pack_lin(g, wm, q + "mlp.fc2", &blk->fc2));
  const OvmTensor* tb; OVM_TRY(g, find_weight(g, wm, q + "attention.relative_position_bias.relative_position_bias_table", -1, &tb));
  if (tb->shape[0] != (2 * ws - 1) * (2 * ws - 1) || tb->shape[1] != nh) { g->err = "relative position bias table shape"; return OVM_ERR_SHAPE; }
  std::vector<float> rb((size_t)nh * ws2 * ws2);
  for (int hh = 0; hh < nh; ++hh)
    for (size_t i = 0; i < (size_t)ws2 * ws2; ++i) rb[(size_t)hh * ws2 * ws2 + i] = tb->data[(size_t)rel_index[i] * nh + hh];
  return upload_f32(g, rb.data(), rb.size(), &blk->relbias);
}

int load_enc_layer(OvmGdino* g, const WeightMap& wm, const std::string& p, EncLayer* ly) {
  const std::string fu = p + "fusion_layer.", te = p + "text_enhancer_layer.", de = p + "deformable_layer.";
  OVM_TRY(g, up_ln(g, wm, fu + "layer_norm_vision", &ly->lnv));
  OVM_TRY(g, up_ln(g, wm, fu + "layer_norm_text", &ly->lnt));
  OVM_TRY(g, pack_cat(g, wm, {fu + "attn.vision_proj", fu + "attn.values_vision_proj"}, &ly->vqv));
  OVM_TRY(g, pack_cat(g, wm, {fu + "attn.text_proj", fu + "attn.values_text_proj"}, &ly->tkv));
  const OvmTensor *gv, *gt; OVM_TRY(g, find_weight(g, wm, fu + "vision_param", -1, &gv)); OVM_TRY(g, find_weight(g, wm, fu + "text_param", -1, &gt));
  OVM_TRY(g, pack_cat(g, wm, {fu + "attn.out_vision_proj"}, &ly->ov, true, gv->data));     // layer scale folded into the projection
  OVM_TRY(g, pack_cat(g, wm, {fu + "attn.out_text_proj"}, &ly->ot, true, gt->data));
  OVM_TRY(g, load_mha(g, wm, te + "self_attn.", g->cfg.heads / 2, &ly->te, false));
  OVM_TRY(g, up_ln(g, wm, te + "layer_norm_before", &ly->te_ln1));
  OVM_TRY(g, up_ln(g, wm, te + "layer_norm_after", &ly->te_ln2));
  OVM_TRY(g, pack_lin(g, wm, te + "fc1", &ly->te_fc1));
  OVM_TRY(g, pack_lin(g, wm, te + "fc2", &ly->te_fc2));
  OVM_TRY(g, load_msda(g, wm, de + "self_attn.", &ly->msda, true));
  OVM_TRY(g, up_ln(g, wm, de + "self_attn_layer_norm", &ly->de_ln1));
  OVM_TRY(g, up_ln(g, wm, de + "final_layer_norm", &ly->de_ln2));
  OVM_TRY(g, pack_lin(g, wm, de + "fc1", &ly->de_fc1));
  return pack_lin(g, wm, de + "fc2", &ly->de_fc2);
}

int load_dec_layer(OvmGdino* g, const WeightMap& wm, const std::string& p, DecLayer* ly) {
  const int heads = g->cfg.heads;
  OVM_TRY(g, load_mha(g, wm, p + "self_attn.", heads, &ly->sa, false, true));
  OVM_TRY(g, up_ln(g, wm, p + "self_attn_layer_norm", &ly->ln1));
  OVM_TRY(g, load_mha(g, wm, p + "encoder_attn_text.", heads, &ly->ca, true, true));
  OVM_TRY(g, up_ln(g, wm, p + "encoder_attn_text_layer_norm", &ly->ln2));
  OVM_TRY(g, load_msda(g, wm, p + "encoder_attn.", &ly->msda, false, true));
  OVM_TRY(g, up_ln(g, wm, p + "encoder_attn_layer_norm", &ly->ln3));
  OVM_TRY(g, pack_lin(g, wm, p + "fc1", &ly->fc1, true, true));
  OVM_TRY(g, pack_lin(g, wm, p + "fc2", &ly->fc2, true, true));
  return up_ln(g, wm, p + "final_layer_norm", &ly->ln4);
}

}  // namespace

int load_bert(OvmGdino* g, const WeightMap& wm) {
  const std::string e = M + "text_backbone.embeddings.";
  const OvmTensor* t; OVM_TRY(g, find_weight(g, wm, e + "word_embeddings.weight", -1, &t));
  g->vocab = (int)t->shape[0]; g->bertD = (int)t->shape[1];
  OVM_TRY(g, upload_weight(g, wm, e + "word_embeddings.weight", -1, &g->word));
  OVM_TRY(g, find_weight(g, wm, e + "position_embeddings.weight", -1, &t)); g->n_pos = (int)t->shape[0];
  OVM_TRY(g, upload_weight(g, wm, e + "position_embeddings.weight", -1, &g->posemb));
  OVM_TRY(g, upload_weight(g, wm, e + "token_type_embeddings.weight", -1, &g->typemb));
  OVM_TRY(g, up_ln(g, wm, e + "LayerNorm", &g->emb_ln));
  for (int i = 0;; ++i) {
    const std::string p = M + "text_backbone.encoder.layer." + std::to_string(i) + ".";
    if (!wm.get(p + "attention.self.query.weight")) break;
    g->bert.emplace_back();
    BertLayer& ly = g->bert.back();
    OVM_TRY(g, pack_cat(g, wm, {p + "attention.self.query", p + "attention.self.key", p + "attention.self.value"}, &ly.qkv));
    OVM_TRY(g, pack_lin(g, wm, p + "attention.output.dense", &ly.ao));
    OVM_TRY(g, up_ln(g, wm, p + "attention.output.LayerNorm", &ly.aln));
    OVM_TRY(g, pack_lin(g, wm, p + "intermediate.dense", &ly.fi));
    OVM_TRY(g, pack_lin(g, wm, p + "output.dense", &ly.fo));
    OVM_TRY(g, up_ln(g, wm, p + "output.LayerNorm", &ly.oln));
  }
  if (g->bertD % g->cfg.bert_heads) { g->err = "bert heads"; return OVM_ERR_INVALID; }
  return pack_lin(g, wm, M + "text_projection", &g->text_proj);
}

int load_swin(OvmGdino* g, const WeightMap& wm) {
  const OvmGdinoConfig& c = g->cfg;
  const std::string bb = M + "backbone.conv_encoder.model.", p = bb + "swin.";
  OVM_TRY(g, pack_conv(g, wm, p + "embeddings.patch_embeddings.projection", &g->pe, nullptr));
  OVM_TRY(g, up_ln(g, wm, p + "embeddings.norm", &g->pe_ln));
  const int ws = c.swin_window, ws2 = ws * ws;
  std::vector<int> rel_index((size_t)ws2 * ws2);
  for (int a = 0; a < ws2; ++a)
    for (int b = 0; b < ws2; ++b) {
      const int dy = a / ws - b / ws + ws - 1, dx = a % ws - b % ws + ws - 1;
      rel_index[(size_t)a * ws2 + b] = dy * (2 * ws - 1) + dx;
    }
  int C = c.swin_embed;
  for (int s = 0; s < 4; ++s) {
    if (c.swin_depths[s] <= 0) break;
    g->stages.emplace_back();
    SwinStage& st = g->stages.back();
    st.nh = c.swin_heads[s]; st.C = C;
    if (C % st.nh || (C / st.nh != 16 && C / st.nh != 32 && C / st.nh != 64)) { g->err = "Swin head dim must be 16, 32 or 64"; return OVM_ERR_SHAPE; }
    const std::string ly = p + "encoder.layers." + std::to_string(s) + ".";
    for (int b = 0; b < c.swin_depths[s]; ++b) {
      st.blocks.emplace_back();
      OVM_TRY(g, load_swin_block(g, wm, ly + "blocks." + std::to_string(b) + ".", C, st.nh, rel_index, &st.blocks.back()));
    }
    if (wm.get(ly + "downsample.reduction.weight")) {
      st.has_red = true;
      OVM_TRY(g, pack_lin(g, wm, ly + "downsample.reduction", &st.red, false));
      OVM_TRY(g, up_ln(g, wm, ly + "downsample.norm", &st.dn));
    }
    const std::string nk = bb + "hidden_states_norms.stage" + std::to_string(s + 1);
    if (wm.get(nk + ".weight")) { st.has_out = true; OVM_TRY(g, up_ln(g, wm, nk, &st.on)); }
    if (st.has_red) C *= 2;
  }
  return OVM_OK;
}

int load_neck(OvmGdino* g, const WeightMap& wm) {
  for (int l = 0; l < g->cfg.n_levels; ++l) {
    const std::string p = M + "input_proj_vision." + std::to_string(l);
    OVM_TRY(g, pack_conv(g, wm, p + ".0", &g->inproj[l].w, &g->inproj[l].k));
    OVM_TRY(g, up_ln(g, wm, p + ".1", &g->inproj[l].gn));
  }
  const OvmTensor* t; OVM_TRY(g, find_weight(g, wm, M + "level_embed", -1, &t));
  g->level_embed.assign(t->data, t->data + numel(t));
  return OVM_OK;
}

int load_encoder(OvmGdino* g, const WeightMap& wm) {
  const OvmGdinoConfig& c = g->cfg;
  for (int i = 0; i < c.enc_layers; ++i) {
    g->enc.emplace_back();
    OVM_TRY(g, load_enc_layer(g, wm, M + "encoder.layers." + std::to_string(i) + ".", &g->enc.back()));
  }
  OVM_TRY(g, pack_lin(g, wm, M + "enc_output", &g->enc_output));
  OVM_TRY(g, up_ln(g, wm, M + "enc_output_norm", &g->enc_output_ln));
  for (int k = 0; k < 3; ++k) OVM_TRY(g, pack_lin(g, wm, M + "encoder_output_bbox_embed.layers." + std::to_string(k), &g->enc_bbox[k]));
  return upload_weight(g, wm, M + "query_position_embeddings.weight", (int64_t)c.num_queries * c.d_model, &g->tgt);
}

int load_decoder(OvmGdino* g, const WeightMap& wm) {
  const OvmGdinoConfig& c = g->cfg;
  std::vector<std::string> kvnames, valnames;
  for (int i = 0; i < c.dec_layers; ++i) {
    const std::string p = M + "decoder.layers." + std::to_string(i) + ".";
    g->dec.emplace_back();
    OVM_TRY(g, load_dec_layer(g, wm, p, &g->dec.back()));
    kvnames.push_back(p + "encoder_attn_text.key"); kvnames.push_back(p + "encoder_attn_text.value");
    valnames.push_back(p + "encoder_attn.value_proj");
  }
  OVM_TRY(g, pack_cat(g, wm, kvnames, &g->dec_kv_text));
  OVM_TRY(g, pack_cat(g, wm, valnames, &g->dec_value));
  OVM_TRY(g, up_ln(g, wm, M + "decoder.layer_norm", &g->dec_ln));
  for (int k = 0; k < 2; ++k) OVM_TRY(g, pack_lin(g, wm, M + "decoder.reference_points_head.layers." + std::to_string(k), &g->ref_head[k], true, true));
  g->bbox.resize(c.dec_layers);
  for (int i = 0; i < c.dec_layers; ++i)
    for (int k = 0; k < 3; ++k) OVM_TRY(g, pack_lin(g, wm, "bbox_embed." + std::to_string(i) + ".layers." + std::to_string(k), &g->bbox[i][k], true, i + 1 < c.dec_layers));
  {
    const int F = c.d_model / 2;
    std::vector<float> dt((size_t)F / 2);
    for (int i = 0; i < F / 2; ++i) dt[i] = powf(10000.0f, 2.f * (float)i / (float)F);       // sine_embed_kernel's dim_t for f / 2 = i
    OVM_TRY(g, upload_f32(g, dt.data(), dt.size(), &g->sine_dim_t));
  }
  // fragment-ordered copies of everything the decoder's row-chain kernels multiply by
  for (int k = 0; k < 2; ++k) OVM_TRY(g, make_frag(g, &g->ref_head[k]));
  for (int i = 0; i < c.dec_layers; ++i) {
    DecLayer& ly = g->dec[i];
    for (Lin* w : {&ly.sa.qk, &ly.sa.v, &ly.sa.out, &ly.ca.q, &ly.ca.out, &ly.msda.offw, &ly.msda.out, &ly.fc1, &ly.fc2}) OVM_TRY(g, make_frag(g, w));
    if (i + 1 < c.dec_layers) for (int k = 0; k < 3; ++k) OVM_TRY(g, make_frag(g, &g->bbox[i][k]));
  }
  return OVM_OK;
}

// [value_proj | sampling_offsets | attention_weights] of every encoder layer as one weight (GdinoTune::enc_fold): the bias covers the
// value columns, that of the other columns lives in the plan's table (plan_offset_tables). The separate packs stay for enc_fold = 0.
int load_encoder_merged(OvmGdino* g, const WeightMap& wm) {
  for (size_t i = 0; i < g->enc.size(); ++i) {
    MsdaW& m = g->enc[i].msda;
    const std::string p = M + "encoder.layers." + std::to_string(i) + ".deformable_layer.self_attn.";
    OVM_TRY(g, pack_cat(g, wm, {p + "value_proj", p + "sampling_offsets", p + "attention_weights"}, &m.voff, false));
    if (m.voff.N != m.value.N + m.offw.N || m.voff.Kpad != m.value.Kpad) { g->err = "merged value | offsets weight shape"; return OVM_ERR_SHAPE; }
    const float* bv; OVM_TRY(g, find_weight(g, wm, p + "value_proj.bias", m.value.N, &bv));
    std::vector<float> b((size_t)m.voff.N, 0.f);
    for (int n = 0; n < m.value.N; ++n) b[n] = bv[n];
    OVM_TRY(g, upload_f32(g, b.data(), b.size(), &m.voff.bias));
  }
  return OVM_OK;
}

}  // namespace gdino
}  // namespace ovm

/* amvhip_pp_mode.c -- amvhip_pp_mode_parse: the reference's pp_get_mode_by_name_and_quality (AMVmuxer/ffmpeg/libpostproc/
 * postprocess.c:744-934) restated for the filters amv_postprocess.hip builds.  Host C, no device.
 *
 * The reference walks the string with strtok: filters between `,` or `/`, a filter's name and options between `:`, empty
 * pieces skipped.  A name of its replace table (`de`, `default`) puts its expansion in front of what is left of the string;
 * here that is a call on the expansion before the walk goes on.  What is not built -- the filters h1 v1 ha va al lb li ci md
 * fd l5 tn and the presets fa / fast / ac -- is AMVHIP_ERR_ARG, and so is everything the reference counts as an error: an
 * unknown name, an option that is neither a letter option nor a number the filter takes. */
#include <stdlib.h>
#include <string.h>

#include "../../include/amvhip.h"

#define PP_BUFFER 500   /* GET_MODE_BUFFER_SIZE */
#define PP_OPTIONS 10   /* OPTIONS_ARRAY_SIZE */

struct pp_filter {
    const char *short_name, *long_name;
    int chrom_default, min_lum_quality, min_chrom_quality;
    int32_t mask;       /* 0: the reference has it, this library does not */
};

static const struct pp_filter filters[] = {
    {"hb", "hdeblock", 1, 1, 3, AMVHIP_PP_H_DEBLOCK}, {"vb", "vdeblock", 1, 2, 4, AMVHIP_PP_V_DEBLOCK},
    {"h1", "x1hdeblock", 1, 1, 3, 0}, {"v1", "x1vdeblock", 1, 2, 4, 0}, {"ha", "ahdeblock", 1, 1, 3, 0}, {"va", "avdeblock", 1, 2, 4, 0},
    {"dr", "dering", 1, 5, 6, AMVHIP_PP_DERING}, {"al", "autolevels", 0, 1, 2, 0}, {"lb", "linblenddeint", 1, 1, 4, 0},
    {"li", "linipoldeint", 1, 1, 4, 0}, {"ci", "cubicipoldeint", 1, 1, 4, 0}, {"md", "mediandeint", 1, 1, 4, 0},
    {"fd", "ffmpegdeint", 1, 1, 4, 0}, {"l5", "lowpass5", 1, 1, 4, 0}, {"tn", "tmpnoise", 1, 7, 8, 0},
    {"fq", "forcequant", 1, 0, 0, AMVHIP_PP_FORCE_QUANT},
};
static const char *const expansion = "hdeblock:a,vdeblock:a,dering:a";

/* the next piece of *p between any of `delims`, empty pieces skipped; terminates it in place */
static char *piece(char **p, const char *delims)
{
    char *s = *p + strspn(*p, delims);
    if (!*s) return *p = s, (char *)0;
    char *e = s + strcspn(s, delims);
    *p = *e ? e + 1 : e;
    *e = 0;
    return s;
}

static int parse_list(const char *list, int quality, amvhip_pp_mode *m)
{
    char temp[PP_BUFFER];
    if (strlen(list) >= sizeof temp) return -1;
    strcpy(temp, list);
    char *rest = temp, *token;
    int error = 0;
    while ((token = piece(&rest, ",/"))) {
        char *name = piece(&token, ":"), *option, *options[PP_OPTIONS];
        int q = 1000000, chrom = -1, luma = -1, enable = 1, unknown = 0, ok = 0;
        if (!name) return -1;
        if (*name == '-') { enable = 0; ++name; }
        while ((option = piece(&token, ":"))) {
            if (!strcmp("autoq", option) || !strcmp("a", option)) q = quality;
            else if (!strcmp("nochrom", option) || !strcmp("y", option)) chrom = 0;
            else if (!strcmp("chrom", option) || !strcmp("c", option)) chrom = 1;
            else if (!strcmp("noluma", option) || !strcmp("n", option)) luma = 0;
            else options[unknown++] = option;
            if (unknown >= PP_OPTIONS - 1) break;
        }
        const int given = unknown;
        if (!strcmp(name, "fast") || !strcmp(name, "fa") || !strcmp(name, "ac")) return -1;
        if (!strcmp(name, "default") || !strcmp(name, "de")) {
            if (parse_list(expansion, quality, m)) return -1;
            ok = 1;
        }
        for (size_t i = 0; i < sizeof filters / sizeof *filters; ++i) {
            const struct pp_filter *f = &filters[i];
            if (strcmp(f->long_name, name) && strcmp(f->short_name, name)) continue;
            if (!f->mask) return -1;
            m->lum_mode &= ~f->mask;
            m->chrom_mode &= ~f->mask;
            ok = 1;
            if (!enable) break;
            if (q >= f->min_lum_quality && luma) m->lum_mode |= f->mask;
            if ((chrom == 1 || (chrom == -1 && f->chrom_default)) && q >= f->min_chrom_quality) m->chrom_mode |= f->mask;
            if (f->mask == AMVHIP_PP_V_DEBLOCK || f->mask == AMVHIP_PP_H_DEBLOCK) {
                for (int o = 0; o < given && o < 2; ++o) {
                    char *tail;
                    const long val = strtol(options[o], &tail, 0);
                    if (tail == options[o]) break;
                    --unknown;
                    if (o == 0) m->base_dc_diff = (int32_t)val;
                    else m->flatness_threshold = (int32_t)val;
                }
            } else if (f->mask == AMVHIP_PP_FORCE_QUANT) {
                m->forced_quant = 15;
                if (given) {
                    char *tail;
                    const long val = strtol(options[0], &tail, 0);
                    if (tail != options[0]) {
                        --unknown;
                        m->forced_quant = (int32_t)val;
                    }
                }
            }
        }
        if (!ok) ++error;
        error += unknown;
    }
    return error ? -1 : 0;
}

int amvhip_pp_mode_parse(const char *name, int quality, amvhip_pp_mode *out)
{
    if (!name || !out) return AMVHIP_ERR_ARG;
    amvhip_pp_mode m = {0, 0, 256 / 8, 56 - 16 - 1, 0};
    if (parse_list(name, quality, &m)) return AMVHIP_ERR_ARG;
    if (!((m.lum_mode | m.chrom_mode) & AMVHIP_PP_FORCE_QUANT)) m.forced_quant = 0;
    *out = m;
    return AMVHIP_OK;
}

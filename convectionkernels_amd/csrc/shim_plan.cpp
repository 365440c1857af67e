// Default Options, the BC7 plans and fine tuning, and a plan from a quality level or from fine tuning (cvtt_mi355x.h): pure host
// functions, no context, no device.
#include <string.h>

#include "cvtt_device.h"
#include "bc7_tables.h"
#include "bc7_quality_events.h"

extern "C"
{
    void cvttmi_default_options(cvttmi_options *out)
    {
        // cvtt::Options::Options(), reference ConvectionKernels.h:89-102
        out->flags = CVTTMI_FLAGS_DEFAULT;
        out->threshold = 0.5f;
        out->redWeight = 0.2125f / 0.7154f;
        out->greenWeight = 1.0f;
        out->blueWeight = 0.0721f / 0.7154f;
        out->alphaWeight = 1.0f;
        out->refineRoundsBC7 = 2;
        out->refineRoundsBC6H = 3;
        out->refineRoundsIIC = 8;
        out->refineRoundsS3TC = 2;
        out->seedPoints = 4;
    }

    void cvttmi_default_bc7_plan(cvttmi_bc7_plan *p)
    {
        // cvtt::BC7EncodingPlan::BC7EncodingPlan(), reference ConvectionKernels.h:166-198:
        // every shape, every partition, four seed points
        memset(p, 0, sizeof(*p));
        p->mode0PartitionEnabled = 0xffff;
        p->mode1PartitionEnabled = p->mode2PartitionEnabled = p->mode3PartitionEnabled = ~0ull;
        p->mode7RGBAPartitionEnabled = p->mode7RGBPartitionEnabled = ~0ull;
        p->mode6Enabled = 1;
        memset(p->mode4SP, 4, sizeof(p->mode4SP));
        memset(p->mode5SP, 4, sizeof(p->mode5SP));
        memset(p->seedPointsForShapeRGB, 4, sizeof(p->seedPointsForShapeRGB));
        memset(p->seedPointsForShapeRGBA, 4, sizeof(p->seedPointsForShapeRGBA));
        for (int i = 0; i < 243; i++)
            p->rgbShapeList[i] = static_cast<uint8_t>(i);
        for (int i = 0; i < 129; i++)
            p->rgbaShapeList[i] = static_cast<uint8_t>(i);
        p->rgbNumShapesToEvaluate = 243;
        p->rgbaNumShapesToEvaluate = 129;
    }

    void cvttmi_default_bc7_fine_tuning(cvttmi_bc7_fine_tuning *p)
    {
        memset(p, 4, sizeof(*p)); // cvtt::BC7FineTuningParams(), ConvectionKernels.h:117-139: four seed points everywhere
    }

    // Shape lists, counts and the mode-7 RGB mask follow from the enables and per-shape seed points
    // (tail of ConfigureBC7EncodingPlanFromFineTuningParams, ConvectionKernels_BC67.cpp:3460-3480).
    static void finishPlan(cvttmi_bc7_plan *plan)
    {
        plan->rgbNumShapesToEvaluate = plan->rgbaNumShapesToEvaluate = 0;
        memset(plan->rgbShapeList, 0, sizeof(plan->rgbShapeList));
        memset(plan->rgbaShapeList, 0, sizeof(plan->rgbaShapeList));
        for (int shape = 0; shape < 243; shape++)
            if (plan->seedPointsForShapeRGB[shape])
                plan->rgbShapeList[plan->rgbNumShapesToEvaluate++] = static_cast<uint8_t>(shape);
        for (int shape = 0; shape < 129; shape++)
            if (plan->seedPointsForShapeRGBA[shape])
                plan->rgbaShapeList[plan->rgbaNumShapesToEvaluate++] = static_cast<uint8_t>(shape);
        plan->mode7RGBPartitionEnabled = plan->mode7RGBAPartitionEnabled & ~plan->mode3PartitionEnabled;
    }

    int cvttmi_bc7_plan_from_fine_tuning(cvttmi_bc7_plan *plan, const cvttmi_bc7_fine_tuning *params)
    {
        if (!plan || !params)
            return CVTTMI_E_INVALID;
        memset(plan, 0, sizeof(*plan));
        // one row per partitioned mode: seed points per partition, number of partitions, subsets, where the enable bit
        // and the per-shape seed points live (modes 0-3 feed the RGB shape set, mode 7 the RGBA set)
        uint64_t m0 = 0;
        const struct
        {
            const uint8_t *sp;
            int numPartitions, numSubsets;
            uint64_t *enable;
            uint8_t *shapeSeeds;
        } rows[5] = {
            {params->mode0SP, 16, 3, &m0, plan->seedPointsForShapeRGB},
            {params->mode1SP, 64, 2, &plan->mode1PartitionEnabled, plan->seedPointsForShapeRGB},
            {params->mode2SP, 64, 3, &plan->mode2PartitionEnabled, plan->seedPointsForShapeRGB},
            {params->mode3SP, 64, 2, &plan->mode3PartitionEnabled, plan->seedPointsForShapeRGB},
            {params->mode7SP, 64, 2, &plan->mode7RGBAPartitionEnabled, plan->seedPointsForShapeRGBA},
        };
        for (const auto &row : rows)
            for (int partition = 0; partition < row.numPartitions; partition++)
            {
                const uint8_t sp = row.sp[partition];
                if (!sp)
                    continue;
                *row.enable |= 1ull << partition;
                for (int subset = 0; subset < row.numSubsets; subset++)
                {
                    const int shape = (row.numSubsets == 3) ? k_shapes3[partition * 3 + subset] : k_shapes2[partition * 2 + subset];
                    if (row.shapeSeeds[shape] < sp)
                        row.shapeSeeds[shape] = sp;
                }
            }
        plan->mode0PartitionEnabled = static_cast<uint16_t>(m0);
        memcpy(plan->mode4SP, params->mode4SP, sizeof(plan->mode4SP));
        memcpy(plan->mode5SP, params->mode5SP, sizeof(plan->mode5SP));
        if (params->mode6SP)
        {
            plan->mode6Enabled = 1;
            if (plan->seedPointsForShapeRGBA[0] < params->mode6SP) // the whole block is shape 0
                plan->seedPointsForShapeRGBA[0] = params->mode6SP;
        }
        finishPlan(plan);
        return CVTTMI_OK;
    }

    int cvttmi_bc7_plan_from_quality(cvttmi_bc7_plan *plan, int quality)
    {
        if (!plan)
            return CVTTMI_E_INVALID;
        quality = quality < 1 ? 1 : quality > 100 ? 100 : quality; // BC67.cpp:3295-3298
        memset(plan, 0, sizeof(*plan));
        uint64_t *masks[5] = {NULL, &plan->mode1PartitionEnabled, &plan->mode2PartitionEnabled, &plan->mode3PartitionEnabled,
                              &plan->mode7RGBAPartitionEnabled};
        uint64_t m0 = 0;
        masks[0] = &m0;
        for (int i = 0; i < CVTT_BC7_NUM_QUALITY_EVENTS; i++)
        {
            const unsigned e = k_bc7QualityEvents[i];
            if (static_cast<int>(e >> 24) > quality)
                break;
            const unsigned kind = (e >> 16) & 255u, index = (e >> 8) & 255u;
            const uint8_t value = static_cast<uint8_t>(e & 255u);
            if (kind < 5)
                *masks[kind] = (*masks[kind] & ~(1ull << index)) | (static_cast<uint64_t>(value & 1u) << index);
            else if (kind == 5)
                plan->mode4SP[index >> 1][index & 1] = value;
            else if (kind == 6)
                plan->mode5SP[index] = value;
            else if (kind == 7)
                plan->mode6Enabled = value;
            else if (kind == 8)
                plan->seedPointsForShapeRGB[index] = value;
            else
                plan->seedPointsForShapeRGBA[index] = value;
        }
        plan->mode0PartitionEnabled = static_cast<uint16_t>(m0);
        finishPlan(plan);
        return CVTTMI_OK;
    }
}
